// a15 gait analysis of the leg tips (the model is this project's own specification, defined in float64 by
// tests/gait_oracle.py): tip position and velocity in leg coordinates, swing/stance by hysteresis, lift-offs, touch-downs and steps,
// the phase of every leg in its step, the coupling of the six phases and the support pattern of every frame.  Every stage is its own
// entry.  No floating-point atomics, every floating-point sum in a fixed order, every integer output exact.  No kernel waits on
// another block of its grid: every scan is three launches (block results, one block per row over the block results with a carry,
// apply).
//
// gait_velocity_kernel: one lane per (frame, leg): tip = q(P4 - P0), vel = q(P4[b] - P4[a]) fps / (b - a) over the clipped window.
// gait_code_kernel: per (frame, leg) the frame's own index where the sample decides (NaN, > on, < off), else -1.
// gait_scan_*: an inclusive int32 max-scan along time of any number of rows of any length: "the last decisive sample at or before t".
//     The rows of one call (the six legs, or the four event series of the six legs) share one grid, blockIdx.y = the row.
// gait_state_kernel: the code of that sample.
// gait_events_kernel: per (frame, leg) four series for the same scan: the last lift-off <= t, the first lift-off >= t (the scan of
//     the reversed series), the last unknown <= t and the last touch-down <= t.
// gait_step_flags_kernel, gait_sum_*, gait_steps_kernel: the lift-offs that start a step, their numbers (the exclusive int32 sum-scan
//     of behaviour_segment.hip over the leg-major flags, so that the rows come out ordered by (leg, t0)), rows and metrics.
// gait_phase_kernel: (t - t0) / (t2 - t0), one division.
// gait_coupling_kernel: a block owns SLICE frames; a lane forms the six unit vectors of a frame once and adds the 21 pairs i <= j
//     (cos(a - b) = ca cb + sa sb is symmetric and sin(a - b) = sa cb - ca sb changes sign exactly, so the other 15 are mirrored
//     when the block writes its [36, 3] partial); lanes combine by a shuffle tree, then the four waves in order.
// gait_coupling_fold_kernel: adds the slices in index order and divides by the count.
// gait_pattern_kernel: the 6-bit mask of every frame; the 64-bin histogram and the per-leg state counts in LDS by integer atomics,
//     added to global memory once per block.
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "common.h"
#include "gait_dev.h"

// Built with -ffp-contract=off (build.py): the tip and the velocity are the oracle's subtractions, products and sums one by one, never
// a fused multiply-add, and the thresholds then see the numbers the bar of the velocity was derived for.

namespace {

using namespace df3d::gait_dev;   // the vectors, the missing rule, the window and the block scan, shared with treadmill.hip

constexpr int EVENT_SERIES = 4;                  // last lift-off, first lift-off (reversed), last unknown, last touch-down
constexpr int SCAN_ROWS = EVENT_SERIES * LEGS;   // the most rows one max-scan call carries
constexpr int SLICE = 2048;                      // frames per block of the coupling: a constant, never the CU count
constexpr int SLICE_PER_LANE = SLICE / THREADS;
constexpr int PAIRS = LEGS * (LEGS + 1) / 2;     // i <= j
constexpr int PATTERNS = 64;
constexpr double TWO_PI = 6.283185307179586476925286766559;

// ------------------------------------------------------------------------------------------------------------------ tip, velocity
__global__ __launch_bounds__(THREADS) void gait_velocity_kernel(const double* __restrict__ pts, long long T, const double* __restrict__ frames,
                                                                int per_frame, double fps, int w, double* __restrict__ tip,
                                                                double* __restrict__ vel) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;   // t * 6 + leg
    if (g >= T * LEGS) return;
    const long long t = g / LEGS;
    const int leg = (int)(g - t * LEGS);
    const int side = leg / 3;
    const size_t coxa = (size_t)coxa_of(leg);   // P0; the tip P4 is four joints on
    const double* F = frames + (per_frame ? (size_t)t * 9 : 0);
    const V3 ex = load3(F), ey = load3(F + 3), ez = load3(F + 6);
    const bool frame_ok = finite3(ex) && finite3(ey) && finite3(ez);
    const double sigma = side ? -1.0 : 1.0;
    const double nan = __builtin_nan("");

    const V3 P0 = load3(pts + ((size_t)t * JOINTS + coxa) * 3), P4 = load3(pts + ((size_t)t * JOINTS + coxa + 4) * 3);
    const V3 r = sub(P4, P0);
    const bool tip_ok = frame_ok && !missing(P0) && !missing(P4);   // selection, never arithmetic on a NaN
    double* tp = tip + (size_t)g * 3;
    tp[0] = tip_ok ? dot(r, ex) : nan;
    tp[1] = tip_ok ? sigma * dot(r, ey) : nan;
    tp[2] = tip_ok ? dot(r, ez) : nan;

    long long a, b;
    window(t, w, T, a, b);
    const V3 Pa = load3(pts + ((size_t)a * JOINTS + coxa + 4) * 3), Pb = load3(pts + ((size_t)b * JOINTS + coxa + 4) * 3);
    const V3 d = sub(Pb, Pa);
    const bool vel_ok = frame_ok && b > a && !missing(Pa) && !missing(Pb);
    const double scale = fps / (double)(b - a);   // one division, as in the oracle
    double* vp = vel + (size_t)g * 3;
    vp[0] = vel_ok ? dot(d, ex) * scale : nan;
    vp[1] = vel_ok ? sigma * dot(d, ey) * scale : nan;
    vp[2] = vel_ok ? dot(d, ez) * scale : nan;
}

// ------------------------------------------------------------------------------------------------------------------ the max-scan
// The inclusive max-scan of v over the block; `exclusive`: that of the lanes before this one (-1 for lane 0); `total`: the block's
// max.  lds: THREADS ints.
__device__ __forceinline__ int block_max_scan(int v, int* lds, int& exclusive, int& total) {
    return block_scan(v, -1, MaxOp(), lds, exclusive, total);
}

// series [rows, T] int32, every entry -1 or its own index.  blockIdx.y = the row.  sums [rows, nb].
__global__ __launch_bounds__(THREADS) void gait_scan_blocks_kernel(const int* __restrict__ in, long long T, int* __restrict__ sums) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int ex, total;
    block_max_scan(i < T ? in[(size_t)blockIdx.y * T + i] : -1, lds, ex, total);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one block per row: the row's block results -> their exclusive max-scan, in place, 256 at a time with a carry
__global__ __launch_bounds__(THREADS) void gait_scan_carry_kernel(int* __restrict__ sums, long long nb) {
    __shared__ int lds[THREADS];
    int* row = sums + (size_t)blockIdx.y * nb;
    int carry = -1;
    for (long long b0 = 0; b0 < nb; b0 += THREADS) {
        const long long b = b0 + threadIdx.x;
        int ex, chunk;
        block_max_scan(b < nb ? row[b] : -1, lds, ex, chunk);
        if (b < nb) row[b] = carry > ex ? carry : ex;
        carry = carry > chunk ? carry : chunk;
    }
}

// out may be in: a lane reads its own entry before it writes it
__global__ __launch_bounds__(THREADS) void gait_scan_apply_kernel(const int* in, long long T, const int* __restrict__ sums, int* out) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int ex, total;
    const int s = block_max_scan(i < T ? in[(size_t)blockIdx.y * T + i] : -1, lds, ex, total);
    const int before = sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
    if (i < T) out[(size_t)blockIdx.y * T + i] = s > before ? s : before;
}

// ------------------------------------------------------------------------------------------------------------------ swing / stance
__device__ __forceinline__ bool decisive(double u, double on, double off) { return isnan(u) || u > on || u < off; }

__global__ __launch_bounds__(THREADS) void gait_code_kernel(const double* __restrict__ vel, long long T, double on, double off, int* __restrict__ last) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int leg = blockIdx.y;
    last[(size_t)leg * T + t] = decisive(vel[((size_t)t * LEGS + leg) * 3], on, off) ? (int)t : -1;
}

__global__ __launch_bounds__(THREADS) void gait_state_kernel(const double* __restrict__ vel, const int* __restrict__ last, long long T, double on,
                                                             int* __restrict__ states) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int leg = blockIdx.y;
    const int j = last[(size_t)leg * T + t];   // -1 or a decisive sample in [0, t]
    int s = -1;
    if (j >= 0) {
        const double u = vel[((size_t)j * LEGS + leg) * 3];
        s = isnan(u) ? -1 : (u > on ? 1 : 0);
    }
    states[(size_t)t * LEGS + leg] = s;
}

// ------------------------------------------------------------------------------------------------------------------ events, steps
// ev [4, 6, T]: series k of leg L is row k * 6 + L.  A state that is neither 0 nor 1 is unknown.
__global__ __launch_bounds__(THREADS) void gait_events_kernel(const int* __restrict__ states, long long T, int* __restrict__ ev) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int leg = blockIdx.y;
    const int s = states[(size_t)t * LEGS + leg];
    const int before = t > 0 ? states[(size_t)(t - 1) * LEGS + leg] : -1;
    const bool lift = before == 0 && s == 1, touch = before == 1 && s == 0, unknown = s != 0 && s != 1;
    const long long r = T - 1 - t;
    ev[(size_t)(0 * LEGS + leg) * T + t] = lift ? (int)t : -1;
    ev[(size_t)(1 * LEGS + leg) * T + r] = lift ? (int)r : -1;
    ev[(size_t)(2 * LEGS + leg) * T + t] = unknown ? (int)t : -1;
    ev[(size_t)(3 * LEGS + leg) * T + t] = touch ? (int)t : -1;
}

// the scanned series
__device__ __forceinline__ int last_lift(const int* ev, long long T, int leg, long long t) { return ev[(size_t)(0 * LEGS + leg) * T + t]; }
__device__ __forceinline__ int last_unknown(const int* ev, long long T, int leg, long long t) { return ev[(size_t)(2 * LEGS + leg) * T + t]; }
__device__ __forceinline__ int last_touch(const int* ev, long long T, int leg, long long t) { return ev[(size_t)(3 * LEGS + leg) * T + t]; }
// the first lift-off at or after t, -1 when there is none (or t is past the end)
__device__ __forceinline__ int first_lift(const int* ev, long long T, int leg, long long t) {
    if (t >= T) return -1;
    const int r = ev[(size_t)(1 * LEGS + leg) * T + (T - 1 - t)];
    return r < 0 ? -1 : (int)(T - 1 - r);
}

// flag [6, T] (leg-major: its sum-scan numbers the steps by (leg, t0)): a lift-off t0 whose next lift-off t2 exists with no unknown
// state in [t0, t2]
__global__ __launch_bounds__(THREADS) void gait_step_flags_kernel(const int* __restrict__ ev, long long T, int* __restrict__ flag) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int leg = blockIdx.y;
    int f = 0;
    if (last_lift(ev, T, leg, t) == (int)t) {
        const int t2 = first_lift(ev, T, leg, t + 1);
        f = t2 >= 0 && last_unknown(ev, T, leg, t2) < (int)t ? 1 : 0;
    }
    flag[(size_t)leg * T + t] = f;
}

// The exclusive scan of v over the block, the block's sum in `total` (the scan of behaviour_segment.hip).  lds: THREADS ints.
__device__ __forceinline__ int block_exclusive_sum(int v, int* lds, int& total) {
    int exclusive;
    block_scan(v, 0, SumOp(), lds, exclusive, total);
    return exclusive;
}

__global__ __launch_bounds__(THREADS) void gait_sum_blocks_kernel(const int* __restrict__ in, long long n, int* __restrict__ sums) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int total;
    block_exclusive_sum(i < n ? in[i] : 0, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums -> their exclusive scan, in place, 256 at a time with a carry; total[0] = the sum of all
__global__ __launch_bounds__(THREADS) void gait_sum_carry_kernel(int* __restrict__ sums, long long nb, int* __restrict__ total) {
    __shared__ int lds[THREADS];
    int carry = 0;
    for (long long b0 = 0; b0 < nb; b0 += THREADS) {
        const long long b = b0 + threadIdx.x;
        int chunk;
        const int ex = block_exclusive_sum(b < nb ? sums[b] : 0, lds, chunk);
        if (b < nb) sums[b] = carry + ex;
        carry += chunk;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ __launch_bounds__(THREADS) void gait_sum_apply_kernel(const int* __restrict__ in, long long n, const int* __restrict__ sums,
                                                                 int* __restrict__ out) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int total;
    const int ex = block_exclusive_sum(i < n ? in[i] : 0, lds, total);
    if (i < n) out[i] = sums[blockIdx.x] + ex;
}

__global__ __launch_bounds__(THREADS) void gait_zero_kernel(unsigned long long* __restrict__ p, long long n) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) p[i] = 0ULL;
}

// steps [3 T, 4] and metrics [3 T, 3] were zeroed; the row of a flagged lift-off is its number
__global__ __launch_bounds__(THREADS) void gait_steps_kernel(const int* __restrict__ ev, const int* __restrict__ flag, const int* __restrict__ number,
                                                             const double* __restrict__ tip, long long T, double fps, long long* __restrict__ steps,
                                                             double* __restrict__ metrics) {
    const long long t0 = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t0 >= T) return;
    const int leg = blockIdx.y;
    if (!flag[(size_t)leg * T + t0]) return;
    const long long t2 = first_lift(ev, T, leg, t0 + 1);   // >= 0: the flag says so
    const long long t1 = last_touch(ev, T, leg, t2);       // the one touch-down between two lift-offs without an unknown state
    const size_t row = (size_t)number[(size_t)leg * T + t0];
    steps[row * 4 + 0] = leg;
    steps[row * 4 + 1] = t0;
    steps[row * 4 + 2] = t1;
    steps[row * 4 + 3] = t2;
    metrics[row * 3 + 0] = (double)(t1 - t0) / fps;
    metrics[row * 3 + 1] = (double)(t2 - t1) / fps;
    metrics[row * 3 + 2] = tip[((size_t)t1 * LEGS + leg) * 3] - tip[((size_t)t0 * LEGS + leg) * 3];   // NaN where either tip is
}

__global__ __launch_bounds__(THREADS) void gait_phase_kernel(const int* __restrict__ ev, long long T, double* __restrict__ phase) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int leg = blockIdx.y;
    double p = __builtin_nan("");
    const int t0 = last_lift(ev, T, leg, t);
    if (t0 >= 0) {
        const int t2 = first_lift(ev, T, leg, t + 1);
        if (t2 >= 0 && last_unknown(ev, T, leg, t2) < t0) p = (double)(t - t0) / (double)(t2 - t0);
    }
    phase[(size_t)t * LEGS + leg] = p;
}

// ------------------------------------------------------------------------------------------------------------------ coupling
__host__ __device__ constexpr int pair_of(int i, int j) { return i * LEGS - i * (i - 1) / 2 + (j - i); }   // i <= j

// part [slices, 36, 3]: per ordered pair the sums of cos and sin of 2 pi (phase_i - phase_j) over the slice's frames where both are
// finite, and their count (exact in a double)
__global__ __launch_bounds__(THREADS) void gait_coupling_kernel(const double* __restrict__ phase, long long T, double* __restrict__ part) {
    __shared__ double red[WAVES][PAIRS * 3];
    double re[PAIRS], im[PAIRS];
    int cnt[PAIRS];
#pragma unroll
    for (int p = 0; p < PAIRS; ++p) {
        re[p] = 0.0;
        im[p] = 0.0;
        cnt[p] = 0;
    }
    const long long t0 = (long long)blockIdx.x * SLICE;
#pragma unroll 1
    for (int k = 0; k < SLICE_PER_LANE; ++k) {
        const long long t = t0 + k * THREADS + threadIdx.x;
        if (t >= T) break;
        double c[LEGS], s[LEGS];
        bool ok[LEGS];
#pragma unroll
        for (int i = 0; i < LEGS; ++i) {
            const double p = phase[(size_t)t * LEGS + i];
            ok[i] = isfinite(p);
            sincos(TWO_PI * (ok[i] ? p : 0.0), &s[i], &c[i]);
        }
#pragma unroll
        for (int i = 0; i < LEGS; ++i)
#pragma unroll
            for (int j = i; j < LEGS; ++j)
                if (ok[i] && ok[j]) {   // selection, never arithmetic on a NaN
                    re[pair_of(i, j)] += c[i] * c[j] + s[i] * s[j];
                    im[pair_of(i, j)] += s[i] * c[j] - c[i] * s[j];
                    cnt[pair_of(i, j)] += 1;
                }
    }
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
#pragma unroll
    for (int p = 0; p < PAIRS; ++p) {
#pragma unroll
        for (int o = df3d::WAVE / 2; o > 0; o >>= 1) {
            re[p] += __shfl_down(re[p], o);
            im[p] += __shfl_down(im[p], o);
            cnt[p] += __shfl_down(cnt[p], o);
        }
        if (lane == 0) {
            red[wave][p * 3 + 0] = re[p];
            red[wave][p * 3 + 1] = im[p];
            red[wave][p * 3 + 2] = (double)cnt[p];
        }
    }
    __syncthreads();
    if (threadIdx.x < LEGS * LEGS * 3) {
        const int k = threadIdx.x / 3, comp = threadIdx.x - 3 * k;
        const int i = k / LEGS, j = k - i * LEGS;
        const int src = (i <= j ? pair_of(i, j) : pair_of(j, i)) * 3 + comp;
        double v = red[0][src];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += red[w][src];
        part[(size_t)blockIdx.x * (LEGS * LEGS * 3) + threadIdx.x] = comp == 1 && i > j ? -v : v;
    }
}

__global__ __launch_bounds__(THREADS) void gait_coupling_fold_kernel(const double* __restrict__ part, int S, double* __restrict__ mean,
                                                                     long long* __restrict__ count) {
    const int k = threadIdx.x;   // the ordered pair
    if (k >= LEGS * LEGS) return;
    double re = 0.0, im = 0.0, n = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* p = part + ((size_t)s * LEGS * LEGS + k) * 3;
        re += p[0];
        im += p[1];
        n += p[2];
    }
    const double nan = __builtin_nan("");
    mean[k * 2 + 0] = n > 0.0 ? re / n : nan;
    mean[k * 2 + 1] = n > 0.0 ? im / n : nan;
    count[k] = (long long)n;
}

// ------------------------------------------------------------------------------------------------------------------ patterns
constexpr int PATTERN_PER_LANE = 8, PATTERN_FRAMES = THREADS * PATTERN_PER_LANE;

// histogram [64] and state_counts [6, 3] (unknown, stance, swing) were zeroed
__global__ __launch_bounds__(THREADS) void gait_pattern_kernel(const int* __restrict__ states, long long T, int* __restrict__ pattern,
                                                               unsigned long long* __restrict__ histogram,
                                                               unsigned long long* __restrict__ state_counts) {
    __shared__ unsigned int local[PATTERNS + LEGS * 3];
    if (threadIdx.x < PATTERNS + LEGS * 3) local[threadIdx.x] = 0u;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * PATTERN_FRAMES;
#pragma unroll 1
    for (int k = 0; k < PATTERN_PER_LANE; ++k) {
        const long long t = t0 + k * THREADS + threadIdx.x;
        if (t >= T) break;
        int mask = 0;
        bool known = true;
#pragma unroll
        for (int leg = 0; leg < LEGS; ++leg) {
            const int s = states[(size_t)t * LEGS + leg];
            const int column = s == 1 ? 2 : (s == 0 ? 1 : 0);
            atomicAdd(&local[PATTERNS + leg * 3 + column], 1u);
            mask |= (s == 1) << leg;
            known = known && column != 0;
        }
        pattern[t] = known ? mask : -1;
        if (known) atomicAdd(&local[mask], 1u);
    }
    __syncthreads();
    if (threadIdx.x < PATTERNS + LEGS * 3) {
        const unsigned int c = local[threadIdx.x];
        if (c) atomicAdd(threadIdx.x < PATTERNS ? &histogram[threadIdx.x] : &state_counts[threadIdx.x - PATTERNS], (unsigned long long)c);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
long long slices_of(long long T) { return (T + SLICE - 1) / SLICE; }

// One workspace layout serves every entry: the scanned series [24, T] and their block results [24, nb], the step flags and their
// numbers [6 T] with the sum-scan's block results, and the coupling's partials [slices, 36, 3].
struct Layout {
    long long series, series_sums, flag, number, flag_sums, coupling, bytes;
};

Layout layout_of(long long T) {
    Layout l;
    l.series = 0;
    l.series_sums = l.series + round64(SCAN_ROWS * T * 4);
    l.flag = l.series_sums + round64(SCAN_ROWS * blocks_of(T) * 4);
    l.number = l.flag + round64(LEGS * T * 4);
    l.flag_sums = l.number + round64(LEGS * T * 4);
    l.coupling = l.flag_sums + round64(blocks_of(LEGS * T) * 4);
    l.bytes = l.coupling + round64(slices_of(T) * LEGS * LEGS * 3 * 8);
    if (l.bytes < 64) l.bytes = 64;   // 0 is the answer for a T outside the range
    return l;
}

// series [rows, T] -> its inclusive max-scan along T, in place
void launch_max_scan(int* series, int rows, long long T, int* sums, hipStream_t st) {
    const dim3 grid(grid_of(T), (unsigned)rows);
    hipLaunchKernelGGL(gait_scan_blocks_kernel, grid, dim3(THREADS), 0, st, series, T, sums);
    hipLaunchKernelGGL(gait_scan_carry_kernel, dim3(1, (unsigned)rows), dim3(THREADS), 0, st, sums, blocks_of(T));
    hipLaunchKernelGGL(gait_scan_apply_kernel, grid, dim3(THREADS), 0, st, series, T, sums, series);
}

// the four scanned event series of `states` in the workspace
int* launch_events(const int* states, long long T, void* work, const Layout& l, hipStream_t st) {
    int* ev = at<int>(work, l.series);
    hipLaunchKernelGGL(gait_events_kernel, dim3(grid_of(T), LEGS), dim3(THREADS), 0, st, states, T, ev);
    launch_max_scan(ev, SCAN_ROWS, T, at<int>(work, l.series_sums), st);
    return ev;
}

#define GAIT_CHECK_T(T) DF3D_CHECK_ARG((T) >= 0 && (T) <= T_MAX, "T must be in [0, (2^31 - 1) / 6]")
#define GAIT_CHECK_WORK(need) DF3D_CHECK_ARG(work_len_bytes >= (need), "work buffer too small (df3d_gait_work_bytes)")

}  // namespace

extern "C" long long df3d_gait_work_bytes(long long T) { return T < 0 || T > T_MAX ? 0 : layout_of(T).bytes; }

extern "C" int df3d_gait_velocity(const double* pts_dev, long long T, const double* frame_dev, long long nframes, double fps, int half_window,
                                  double* tip_dev, double* vel_dev, void* stream) {
    GAIT_CHECK_T(T);
    DF3D_CHECK_ARG(std::isfinite(fps) && fps > 0.0, "fps must be finite and > 0");
    DF3D_CHECK_ARG(half_window >= HALF_MIN && half_window <= HALF_MAX, "half_window must be in [1, 64]");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(nframes == 1 || nframes == T, "nframes must be 1 (one frame for the recording) or T (one per pose)");
    DF3D_BUFFERS({"pts", pts_dev, T * JOINTS * 24, 8}, {"frame", frame_dev, nframes * 72, 8}, {"tip", tip_dev, T * LEGS * 24, 8},
                 {"vel", vel_dev, T * LEGS * 24, 8});
    hipLaunchKernelGGL(gait_velocity_kernel, dim3(grid_of(T * LEGS)), dim3(THREADS), 0, df3d::as_stream(stream), pts_dev, T, frame_dev,
                       nframes != 1 ? 1 : 0, fps, half_window, tip_dev, vel_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_gait_states(const double* vel_dev, long long T, double on, double off, int* states_dev, void* work_dev, long long work_len_bytes,
                                void* stream) {
    GAIT_CHECK_T(T);
    DF3D_CHECK_ARG(std::isfinite(on) && std::isfinite(off), "on and off must be finite");
    DF3D_CHECK_ARG(on > off, "on must be above off");
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    GAIT_CHECK_WORK(l.bytes);
    DF3D_BUFFERS({"vel", vel_dev, T * LEGS * 24, 8}, {"states", states_dev, T * LEGS * 4, 4}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    int* last = at<int>(work_dev, l.series);
    const dim3 grid(grid_of(T), LEGS);
    hipLaunchKernelGGL(gait_code_kernel, grid, dim3(THREADS), 0, st, vel_dev, T, on, off, last);
    launch_max_scan(last, LEGS, T, at<int>(work_dev, l.series_sums), st);
    hipLaunchKernelGGL(gait_state_kernel, grid, dim3(THREADS), 0, st, vel_dev, last, T, on, states_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_gait_steps(const int* states_dev, const double* tip_dev, long long T, double fps, long long* steps_dev, double* metrics_dev,
                               int* num_steps_dev, void* work_dev, long long work_len_bytes, void* stream) {
    GAIT_CHECK_T(T);
    DF3D_CHECK_ARG(std::isfinite(fps) && fps > 0.0, "fps must be finite and > 0");
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    GAIT_CHECK_WORK(l.bytes);
    const long long rows = 3 * T;   // a leg lifts off at most every other frame
    DF3D_BUFFERS({"states", states_dev, T * LEGS * 4, 4}, {"tip", tip_dev, T * LEGS * 24, 8}, {"steps", steps_dev, rows * 32, 8},
                 {"metrics", metrics_dev, rows * 24, 8}, {"num_steps", num_steps_dev, 4, 4}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    const int* ev = launch_events(states_dev, T, work_dev, l, st);
    int *flag = at<int>(work_dev, l.flag), *number = at<int>(work_dev, l.number), *sums = at<int>(work_dev, l.flag_sums);
    const dim3 grid(grid_of(T), LEGS);
    hipLaunchKernelGGL(gait_step_flags_kernel, grid, dim3(THREADS), 0, st, ev, T, flag);
    const long long n = LEGS * T;
    hipLaunchKernelGGL(gait_sum_blocks_kernel, dim3(grid_of(n)), dim3(THREADS), 0, st, flag, n, sums);
    hipLaunchKernelGGL(gait_sum_carry_kernel, dim3(1), dim3(THREADS), 0, st, sums, blocks_of(n), num_steps_dev);
    hipLaunchKernelGGL(gait_sum_apply_kernel, dim3(grid_of(n)), dim3(THREADS), 0, st, flag, n, sums, number);
    hipLaunchKernelGGL(gait_zero_kernel, dim3(grid_of(rows * 4)), dim3(THREADS), 0, st, reinterpret_cast<unsigned long long*>(steps_dev), rows * 4);
    hipLaunchKernelGGL(gait_zero_kernel, dim3(grid_of(rows * 3)), dim3(THREADS), 0, st, reinterpret_cast<unsigned long long*>(metrics_dev), rows * 3);
    hipLaunchKernelGGL(gait_steps_kernel, grid, dim3(THREADS), 0, st, ev, flag, number, tip_dev, T, fps, steps_dev, metrics_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_gait_phase(const int* states_dev, long long T, double* phase_dev, void* work_dev, long long work_len_bytes, void* stream) {
    GAIT_CHECK_T(T);
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    GAIT_CHECK_WORK(l.bytes);
    DF3D_BUFFERS({"states", states_dev, T * LEGS * 4, 4}, {"phase", phase_dev, T * LEGS * 8, 8}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    const int* ev = launch_events(states_dev, T, work_dev, l, st);
    hipLaunchKernelGGL(gait_phase_kernel, dim3(grid_of(T), LEGS), dim3(THREADS), 0, st, ev, T, phase_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_gait_coupling(const double* phase_dev, long long T, double* mean_dev, long long* count_dev, void* work_dev,
                                  long long work_len_bytes, void* stream) {
    GAIT_CHECK_T(T);
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    GAIT_CHECK_WORK(l.bytes);
    DF3D_BUFFERS({"phase", phase_dev, T * LEGS * 8, 8}, {"mean", mean_dev, LEGS * LEGS * 16, 8}, {"count", count_dev, LEGS * LEGS * 8, 8},
                 {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    double* part = at<double>(work_dev, l.coupling);
    const int S = (int)slices_of(T);
    hipLaunchKernelGGL(gait_coupling_kernel, dim3((unsigned)S), dim3(THREADS), 0, st, phase_dev, T, part);
    hipLaunchKernelGGL(gait_coupling_fold_kernel, dim3(1), dim3(THREADS), 0, st, part, S, mean_dev, count_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_gait_patterns(const int* states_dev, long long T, int* pattern_dev, long long* histogram_dev, long long* state_counts_dev,
                                  void* stream) {
    GAIT_CHECK_T(T);
    if (T == 0) return DF3D_OK;
    DF3D_BUFFERS({"states", states_dev, T * LEGS * 4, 4}, {"pattern", pattern_dev, T * 4, 4}, {"histogram", histogram_dev, PATTERNS * 8, 8},
                 {"state_counts", state_counts_dev, LEGS * 3 * 8, 8});
    hipStream_t st = df3d::as_stream(stream);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(histogram_dev);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(state_counts_dev);
    hipLaunchKernelGGL(gait_zero_kernel, dim3(1), dim3(THREADS), 0, st, hist, (long long)PATTERNS);
    hipLaunchKernelGGL(gait_zero_kernel, dim3(1), dim3(THREADS), 0, st, counts, (long long)(LEGS * 3));
    hipLaunchKernelGGL(gait_pattern_kernel, dim3((unsigned)((T + PATTERN_FRAMES - 1) / PATTERN_FRAMES)), dim3(THREADS), 0, st, states_dev, T, pattern_dev,
                       hist, counts);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
