// a16 repair of the 3-D pose (the model is this project's own specification, defined in float64 by
// tests/pose_repair_oracle.py): a Hampel test of every joint against the median of its own window, then linear filling of the short
// gaps that missing joints and outliers leave.  No floating-point atomics, every output exact: two runs give the same bits, and the
// bits are the oracle's.  No kernel waits on another block of its grid and nothing depends on the CU count.
//
// repair_outliers_kernel: a block owns one joint and TILE consecutive frames.  It brings x[tile - h, tile + TILE + h) of the three
//     coordinates into LDS once, coordinate-major, with one validity byte per sample; a lane's window is then a run of consecutive
//     8-byte words and the lanes of a wave read consecutive addresses.  A lane folds the validity of its window into a 129-bit mask
//     and takes the two middle order statistics of the valid samples by counting ranks, ties broken by index: exactly one sample has
//     each rank, so the value is that of a sort.  The same select runs on |x - m|, formed as it is read.  An invalid sample is
//     excluded by its mask bit, never by arithmetic on a NaN: its place in LDS holds zeros.
// repair_good_kernel: per (frame, joint) two series for the max-scan: the frame's own index where the joint is good (flags == 0),
//     else -1, and the same on the reversed index.
// repair_scan_*: the inclusive int32 max-scan of csrc/gait.hip (block results, one block per row over them with a carry, apply), a
//     copy: gait.hip's object stays what it was, and its resource report names its own kernels.
// repair_fill_kernel: one lane per (frame, joint) in the pose's own order, so that points, flags, output and status are read and
//     written in runs; only a bad joint reads the two scanned series.  The counts go to LDS by integer atomics and to global memory
//     once per block of 2 048 pairs.
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "common.h"

// Built with -ffp-contract=off (build.py): the deviation, the threshold, the score and the filled value are the oracle's
// subtractions, products, divisions and sums one by one, never a fused multiply-add, and compare bit for bit.

namespace {

constexpr int THREADS = 256;
constexpr int TILE = THREADS;                    // frames per block of the outlier test: one lane per frame
constexpr int JOINTS = 38;
constexpr int CODES = 5;                         // kept, missing filled, outlier filled, missing left, outlier removed
constexpr int HALF_MIN = 1, HALF_MAX = 64;
constexpr int SPAN = TILE + 2 * HALF_MAX;        // the samples a block holds at the widest window
constexpr int MAX_GAP_MAX = 1000000;
constexpr int SCAN_ROWS = 2 * JOINTS;            // last good <= t, and first good >= t as the scan of the reversed series
constexpr long long T_MAX = 0x7fffffffLL / JOINTS;

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 load3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ bool finite3(V3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// section 14's rule: all three coordinates exactly zero (the DLT's "fewer than two views"), or any of them not finite
__device__ __forceinline__ bool missing(V3 p) { return (p.x == 0.0 && p.y == 0.0 && p.z == 0.0) || !finite3(p); }

// ------------------------------------------------------------------------------------------------------------------ outliers
// the validity of a window of up to 2 * 64 + 1 samples
struct Mask {
    unsigned long long lo, hi;
    bool top;
    __device__ __forceinline__ bool at(int l) const { return l < 64 ? (lo >> l) & 1ULL : (l < 128 ? (hi >> (l - 64)) & 1ULL : top); }
};

// The order statistics k1 <= k2 <= k1 + 1 of the valid samples among x[0, W) -- with DEV of |x - centre| -- by counting ranks:
// rank(i) = the valid samples below sample i, or equal to it and before it.  x points into LDS.
// The valid samples among x[l, end) that lie below vi -- with TIES: or equal to it --; bit 0 of m is sample l's validity, and m
// leaves shifted down to sample `end`.  Straight-line: one read, one comparison, the mask bit by a bitwise and, one shift.
template <bool DEV, bool TIES>
__device__ __forceinline__ int count_below(const double* x, int l, int end, unsigned long long& m, double centre, double vi) {
    int n = 0;
    for (; l < end; ++l, m >>= 1) {
        const double vl = DEV ? fabs(x[l] - centre) : x[l];
        n += (int)(m & 1ULL) & (int)(TIES ? vl <= vi : vl < vi);
    }
    return n;
}

// the rank of sample i, whose value is vi: ties count before i and not from i on (i is uniform over the wave)
template <bool DEV>
__device__ __forceinline__ int rank_of(const double* x, int W, const Mask& mask, double centre, double vi, int i) {
    int rank = 0;
    for (int l0 = 0; l0 < W; l0 += 64) {
        unsigned long long m = l0 == 0 ? mask.lo : (l0 == 64 ? mask.hi : (unsigned long long)mask.top);
        const int l1 = W < l0 + 64 ? W : l0 + 64;
        const int mid = i < l0 ? l0 : (i > l1 ? l1 : i);
        rank += count_below<DEV, true>(x, l0, mid, m, centre, vi);
        rank += count_below<DEV, false>(x, mid, l1, m, centre, vi);
    }
    return rank;
}

template <bool DEV>
__device__ __forceinline__ void select_pair(const double* x, int W, const Mask& mask, double centre, int k1, int k2, double& v1, double& v2) {
    v1 = v2 = 0.0;
    int found = 0;
    for (int i = 0; i < W && found < 2; ++i) {
        if (!mask.at(i)) continue;
        const double vi = DEV ? fabs(x[i] - centre) : x[i];
        const int rank = rank_of<DEV>(x, W, mask, centre, vi, i);
        if (rank == k1) {
            v1 = vi;
            ++found;
        }
        if (rank == k2) {
            v2 = vi;
            ++found;
        }
    }
}

// v_(n-1)/2 for an odd count, the mean of the two middle ones for an even count
__device__ __forceinline__ double median_of(double v1, double v2, bool odd) { return odd ? v1 : (v1 + v2) * 0.5; }

// flags [T, 38]: bit 0 missing, bit 1 outlier.  score [T, 38] or null.  grid (tiles, 38).
__global__ __launch_bounds__(THREADS) void repair_outliers_kernel(const double* __restrict__ pts, long long T, int h, double scale, double floor,
                                                                  int n_min, unsigned char* __restrict__ flags, double* __restrict__ score) {
    __shared__ double xs[3][SPAN];
    __shared__ unsigned char valid[SPAN];
    const int j = blockIdx.y;
    const long long tile0 = (long long)blockIdx.x * TILE;
    for (int p = threadIdx.x; p < TILE + 2 * h; p += THREADS) {   // p < SPAN: h <= HALF_MAX
        const long long s = tile0 - h + p;
        V3 P = {0.0, 0.0, 0.0};
        bool good = false;
        if (s >= 0 && s < T) {
            P = load3(pts + ((size_t)s * JOINTS + j) * 3);
            good = !missing(P);
        }
        if (!good) P = {0.0, 0.0, 0.0};   // every number in LDS is finite: a masked-out sample is dropped by its bit, after finite arithmetic
        xs[0][p] = P.x;
        xs[1][p] = P.y;
        xs[2][p] = P.z;
        valid[p] = good ? 1 : 0;
    }
    __syncthreads();
    const long long t = tile0 + threadIdx.x;
    if (t >= T) return;
    const int base = threadIdx.x, W = 2 * h + 1;   // the window of frame t is [base, base + W) of the block's samples, t itself at base + h
    const size_t g = (size_t)t * JOINTS + j;
    const double nan = __builtin_nan("");
    if (!valid[base + h]) {
        flags[g] = 1;
        if (score) score[g] = nan;
        return;
    }
    Mask mask = {0ULL, 0ULL, false};
    int n = 0;
    for (int l = 0; l < W; ++l) {
        const bool v = valid[base + l] != 0;   // a frame outside the recording is not valid: the clipped window
        n += v ? 1 : 0;
        if (l < 64)
            mask.lo |= (unsigned long long)v << l;
        else if (l < 128)
            mask.hi |= (unsigned long long)v << (l - 64);
        else
            mask.top = v;
    }
    if (n < n_min) {   // untested
        flags[g] = 0;
        if (score) score[g] = nan;
        return;
    }
    const int k1 = (n - 1) / 2, k2 = n / 2;
    const bool odd = k1 == k2;
    bool outlier = false;
    double best = 0.0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        const double* x = &xs[c][base];
        double v1, v2;
        select_pair<false>(x, W, mask, 0.0, k1, k2, v1, v2);
        const double m = median_of(v1, v2, odd);
        select_pair<true>(x, W, mask, m, k1, k2, v1, v2);
        const double mad = median_of(v1, v2, odd);
        const double dev = fabs(x[h] - m);
        const double product = scale * mad;
        const double thr = product > floor ? product : floor;
        outlier = outlier || dev > thr;
        const double r = dev == 0.0 ? 0.0 : (thr == 0.0 ? __builtin_inf() : dev / thr);
        if (c == 0 || r > best) best = r;
    }
    flags[g] = outlier ? 2 : 0;
    if (score) score[g] = best;
}

// ------------------------------------------------------------------------------------------------------------------ the max-scan
// series [76, T]: row j the good frames of joint j, row 38 + j the same on the reversed index
__global__ __launch_bounds__(THREADS) void repair_good_kernel(const unsigned char* __restrict__ flags, long long T, int* __restrict__ series) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const int j = blockIdx.y;
    const bool good = flags[(size_t)t * JOINTS + j] == 0;
    const long long r = T - 1 - t;
    series[(size_t)j * T + t] = good ? (int)t : -1;
    series[(size_t)(JOINTS + j) * T + r] = good ? (int)r : -1;
}

// The inclusive max-scan of v over the block; `exclusive`: that of the lanes before this one (-1 for lane 0); `total`: the block's
// max.  lds: THREADS ints.
__device__ __forceinline__ int block_max_scan(int v, int* lds, int& exclusive, int& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    int s = v;
    for (int o = 1; o < THREADS; o <<= 1) {
        const int other = t >= o ? lds[t - o] : -1;
        __syncthreads();
        s = s > other ? s : other;
        lds[t] = s;
        __syncthreads();
    }
    exclusive = t ? lds[t - 1] : -1;
    total = lds[THREADS - 1];
    __syncthreads();   // the next call may write lds
    return s;
}

// series [rows, T] int32, every entry -1 or its own index.  blockIdx.y = the row.  sums [rows, nb].
__global__ __launch_bounds__(THREADS) void repair_scan_blocks_kernel(const int* __restrict__ in, long long T, int* __restrict__ sums) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int ex, total;
    block_max_scan(i < T ? in[(size_t)blockIdx.y * T + i] : -1, lds, ex, total);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one block per row: the row's block results -> their exclusive max-scan, in place, 256 at a time with a carry
__global__ __launch_bounds__(THREADS) void repair_scan_carry_kernel(int* __restrict__ sums, long long nb) {
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
__global__ __launch_bounds__(THREADS) void repair_scan_apply_kernel(const int* in, long long T, const int* __restrict__ sums, int* out) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int ex, total;
    const int s = block_max_scan(i < T ? in[(size_t)blockIdx.y * T + i] : -1, lds, ex, total);
    const int before = sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
    if (i < T) out[(size_t)blockIdx.y * T + i] = s > before ? s : before;
}

// ------------------------------------------------------------------------------------------------------------------ gaps
__global__ __launch_bounds__(THREADS) void repair_zero_kernel(unsigned long long* __restrict__ p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0ULL;
}

constexpr int FILL_PER_LANE = 8, FILL_ITEMS = THREADS * FILL_PER_LANE;   // (frame, joint) pairs per block: 190 global atomics for 2 048

// series: the scanned rows of repair_good_kernel.  counts [38, 5] was zeroed.
__global__ __launch_bounds__(THREADS) void repair_fill_kernel(const double* __restrict__ pts, const unsigned char* __restrict__ flags,
                                                              const int* __restrict__ series, long long T, int max_gap, double* __restrict__ out,
                                                              signed char* __restrict__ status, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int local[JOINTS * CODES];
    if (threadIdx.x < JOINTS * CODES) local[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < FILL_PER_LANE; ++k) {
        const long long g = (long long)blockIdx.x * FILL_ITEMS + k * THREADS + threadIdx.x;   // t * 38 + j
        if (g >= T * JOINTS) break;
        const long long t = g / JOINTS;
        const int j = (int)(g - t * JOINTS);
        const unsigned char f = flags[g];
        V3 Y = load3(pts + (size_t)g * 3);   // a good joint keeps its bits
        int code = 0;
        if (f) {
            const int a = series[(size_t)j * T + t];                         // the last good frame before t, or -1
            const int r = series[(size_t)(JOINTS + j) * T + (T - 1 - t)];   // the same on the reversed index
            const long long b = r < 0 ? -1 : T - 1 - r;                     // the first good frame after t, or -1
            const bool filled = a >= 0 && b >= 0 && b - a - 1 <= (long long)max_gap;
            if (filled) {
                const V3 A = load3(pts + ((size_t)a * JOINTS + j) * 3), B = load3(pts + ((size_t)b * JOINTS + j) * 3);
                const double w = (double)(t - a) / (double)(b - a);   // one division
                Y = {A.x + (B.x - A.x) * w, A.y + (B.y - A.y) * w, A.z + (B.z - A.z) * w};
            } else {
                Y = {0.0, 0.0, 0.0};   // missing by the project's rule
            }
            code = (f & 1) ? (filled ? 1 : 3) : (filled ? 2 : 4);
        }
        double* o = out + (size_t)g * 3;
        o[0] = Y.x;
        o[1] = Y.y;
        o[2] = Y.z;
        status[g] = (signed char)code;
        atomicAdd(&local[j * CODES + code], 1u);
    }
    __syncthreads();
    if (threadIdx.x < JOINTS * CODES) {
        const unsigned int c = local[threadIdx.x];
        if (c) atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
long long round64(long long b) { return (b + 63) / 64 * 64; }
long long blocks_of(long long n) { return (n + THREADS - 1) / THREADS; }
unsigned grid_of(long long n) { return (unsigned)blocks_of(n); }

// the scanned series [76, T] and their block results [76, nb]
struct Layout {
    long long series, sums, bytes;
};

Layout layout_of(long long T) {
    Layout l;
    l.series = 0;
    l.sums = l.series + round64(SCAN_ROWS * T * 4);
    l.bytes = l.sums + round64(SCAN_ROWS * blocks_of(T) * 4);
    if (l.bytes < 64) l.bytes = 64;   // 0 is the answer for a T outside the range
    return l;
}

template <typename P>
P* at(void* work, long long offset) {
    return reinterpret_cast<P*>(static_cast<char*>(work) + offset);
}

#define REPAIR_CHECK_T(T) DF3D_CHECK_ARG((T) >= 0 && (T) <= T_MAX, "T must be in [0, (2^31 - 1) / 38]")

}  // namespace

extern "C" long long df3d_repair_work_bytes(long long T) { return T < 0 || T > T_MAX ? 0 : layout_of(T).bytes; }

extern "C" int df3d_repair_outliers(const double* pts_dev, long long T, int half_window, double scale, double floor, int min_count,
                                    unsigned char* flags_dev, double* score_dev, void* stream) {
    REPAIR_CHECK_T(T);
    DF3D_CHECK_ARG(half_window >= HALF_MIN && half_window <= HALF_MAX, "half_window must be in [1, 64]");
    DF3D_CHECK_ARG(std::isfinite(scale) && scale > 0.0, "scale must be finite and > 0");
    DF3D_CHECK_ARG(std::isfinite(floor) && floor >= 0.0, "floor must be finite and >= 0");
    DF3D_CHECK_ARG(min_count >= 1 && min_count <= 2 * half_window + 1, "min_count must be in [1, 2 half_window + 1]");
    if (T == 0) return DF3D_OK;
    if (score_dev)
        DF3D_BUFFERS({"pts", pts_dev, T * JOINTS * 24, 8}, {"flags", flags_dev, T * JOINTS, 1}, {"score", score_dev, T * JOINTS * 8, 8});
    else
        DF3D_BUFFERS({"pts", pts_dev, T * JOINTS * 24, 8}, {"flags", flags_dev, T * JOINTS, 1});
    hipLaunchKernelGGL(repair_outliers_kernel, dim3(grid_of(T), JOINTS), dim3(THREADS), 0, df3d::as_stream(stream), pts_dev, T, half_window, scale,
                       floor, min_count, flags_dev, score_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_repair_fill(const double* pts_dev, const unsigned char* flags_dev, long long T, int max_gap, double* out_dev,
                                signed char* status_dev, long long* counts_dev, void* work_dev, long long work_len_bytes, void* stream) {
    REPAIR_CHECK_T(T);
    DF3D_CHECK_ARG(max_gap >= 0 && max_gap <= MAX_GAP_MAX, "max_gap must be in [0, 1000000]");
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    DF3D_CHECK_ARG(work_len_bytes >= l.bytes, "work buffer too small (df3d_repair_work_bytes)");
    DF3D_BUFFERS({"pts", pts_dev, T * JOINTS * 24, 8}, {"flags", flags_dev, T * JOINTS, 1}, {"out", out_dev, T * JOINTS * 24, 8},
                 {"status", status_dev, T * JOINTS, 1}, {"counts", counts_dev, JOINTS * CODES * 8, 8}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    int *series = at<int>(work_dev, l.series), *sums = at<int>(work_dev, l.sums);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_dev);
    const dim3 rows(grid_of(T), SCAN_ROWS);
    hipLaunchKernelGGL(repair_good_kernel, dim3(grid_of(T), JOINTS), dim3(THREADS), 0, st, flags_dev, T, series);
    hipLaunchKernelGGL(repair_scan_blocks_kernel, rows, dim3(THREADS), 0, st, series, T, sums);
    hipLaunchKernelGGL(repair_scan_carry_kernel, dim3(1, SCAN_ROWS), dim3(THREADS), 0, st, sums, blocks_of(T));
    hipLaunchKernelGGL(repair_scan_apply_kernel, rows, dim3(THREADS), 0, st, series, T, sums, series);
    hipLaunchKernelGGL(repair_zero_kernel, dim3(1), dim3(THREADS), 0, st, counts, JOINTS * CODES);
    hipLaunchKernelGGL(repair_fill_kernel, dim3((unsigned)((T * JOINTS + FILL_ITEMS - 1) / FILL_ITEMS)), dim3(THREADS), 0, st, pts_dev, flags_dev, series, T, max_gap, out_dev,
                       status_dev, counts);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
