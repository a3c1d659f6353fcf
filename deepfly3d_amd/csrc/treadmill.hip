// a17 the treadmill ball and the fictive walking path from the stance tips (the model is this project's own
// specification, defined in float64 by tests/treadmill_oracle.py): the tips and their velocities in the recording's body frame, one
// sphere through the stance samples, the ball's rotation in every frame, and the path the fly would have walked.  No floating-point
// atomics, every floating-point sum in a fixed order, every integer output exact.  No kernel waits on another block of its grid.
//
// ball_tips_kernel: one lane per (frame, leg): b = F (P4 - o) with o the mean of the six coxa medians, v = F (P4[hi] - P4[lo]) fps /
//     (hi - lo) over gait's clipped window.
// ball_sums_kernel<MODE>: a block owns SLICE samples (t, L) of the flattened [6 T]; a lane adds its eight in order, lanes combine by a
//     shuffle tree, then the four waves in order: part [slices, PART].  MODE 0: the count and the sum of b; MODE 1: the 13 sums of the
//     centred 4 x 4 normal equations; MODE 2: the 9 sums of the 3 x 3 Gauss-Newton normal equations and the sum of squared residuals.
// ball_mean_kernel, ball_algebraic_kernel, ball_step_kernel: one wave each: lane k adds sum k over the slices in index order, lane 0
//     solves by Cholesky and leaves the parameters in the workspace; the last writes centre, radius, rms, count and status.
// ball_rotation_kernel: one lane per frame: the 3 x 3 system of the stance legs, its Cholesky solve, the residual and the fictive motion.
// path_*: the two exclusive prefix sums (theta, then x and y), each three launches of gait_dev.h's block scan with the terms formed on
//     the fly: block results, one block per row over the block results with a carry, apply.
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "common.h"
#include "gait_dev.h"

// Built with -ffp-contract=off (build.py): tips, velocities and the slice sums are the oracle's operations one by one, compared bit for
// bit; the bars of the solved quantities count those roundings.

namespace {

using namespace df3d::gait_dev;

constexpr int SLICE = 2048;                       // samples (t, L) per block of a sum: a constant, never the CU count
constexpr int SLICE_PER_LANE = SLICE / THREADS;
constexpr int PART = 16;                          // doubles per slice partial, the most a mode sums (13)
constexpr int SUMS_COUNT = 4, SUMS_ALGEBRAIC = 13, SUMS_STEP = 10;
constexpr int SUMS_OUT = SUMS_COUNT + SUMS_ALGEBRAIC;   // what df3d_ball_fit reports of its sums
constexpr int ITER_MIN = 1, ITER_MAX = 64;
constexpr int LEGS_MIN = 2;
constexpr int STATUS_REFUSED = 1, STATUS_START_BELOW = 2;
// the workspace's parameter block, doubles
constexpr int P_MEAN = 0, P_COUNT = 3, P_CENTER = 4, P_RADIUS = 7, P_STATUS = 8, P_DOUBLES = 64;

// ------------------------------------------------------------------------------------------------------------------ tips, velocities
__global__ __launch_bounds__(THREADS) void ball_tips_kernel(const double* __restrict__ pts, long long T, const double* __restrict__ frame,
                                                            const double* __restrict__ coxa, double fps, int w, double* __restrict__ tip,
                                                            double* __restrict__ vel) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;   // t * 6 + leg
    if (g >= T * LEGS) return;
    const long long t = g / LEGS;
    const int leg = (int)(g - t * LEGS);
    const size_t p4 = (size_t)coxa_of(leg) + 4;
    const V3 ex = load3(frame), ey = load3(frame + 3), ez = load3(frame + 6);
    V3 o = load3(coxa);   // the six medians in leg order, then one division
#pragma unroll
    for (int k = 1; k < LEGS; ++k) {
        const V3 m = load3(coxa + 3 * k);
        o = {o.x + m.x, o.y + m.y, o.z + m.z};
    }
    o = {o.x / 6.0, o.y / 6.0, o.z / 6.0};
    const bool frame_ok = finite3(ex) && finite3(ey) && finite3(ez) && finite3(o);
    const double nan = __builtin_nan("");

    const V3 P4 = load3(pts + ((size_t)t * JOINTS + p4) * 3);
    const V3 r = sub(P4, o);
    const bool tip_ok = frame_ok && !missing(P4);   // selection, never arithmetic on a NaN
    double* tp = tip + (size_t)g * 3;
    tp[0] = tip_ok ? dot(r, ex) : nan;
    tp[1] = tip_ok ? dot(r, ey) : nan;
    tp[2] = tip_ok ? dot(r, ez) : nan;

    long long a, b;
    window(t, w, T, a, b);
    const V3 Pa = load3(pts + ((size_t)a * JOINTS + p4) * 3), Pb = load3(pts + ((size_t)b * JOINTS + p4) * 3);
    const V3 d = sub(Pb, Pa);
    const bool vel_ok = frame_ok && b > a && !missing(Pa) && !missing(Pb);
    const double scale = fps / (double)(b - a);   // one division, as in the oracle
    double* vp = vel + (size_t)g * 3;
    vp[0] = vel_ok ? dot(d, ex) * scale : nan;
    vp[1] = vel_ok ? dot(d, ey) * scale : nan;
    vp[2] = vel_ok ? dot(d, ez) * scale : nan;
}

// ------------------------------------------------------------------------------------------------------------------ the slice sums
template <int MODE>
struct Sums;
template <>
struct Sums<0> {
    static constexpr int N = SUMS_COUNT;
};
template <>
struct Sums<1> {
    static constexpr int N = SUMS_ALGEBRAIC;
};
template <>
struct Sums<2> {
    static constexpr int N = SUMS_STEP;
};

// tip [6 T, 3], states [6 T]; a sample is a stance state with a finite tip.  par: the workspace's parameter block.
template <int MODE>
__global__ __launch_bounds__(THREADS) void ball_sums_kernel(const double* __restrict__ tip, const int* __restrict__ states, long long n,
                                                            const double* __restrict__ par, double* __restrict__ part) {
    constexpr int N = Sums<MODE>::N;
    __shared__ double red[WAVES][PART];
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    const V3 ref = MODE == 0 ? V3{0.0, 0.0, 0.0} : load3(par + (MODE == 1 ? P_MEAN : P_CENTER));
    const double R = MODE == 2 ? par[P_RADIUS] : 0.0;
    const long long i0 = (long long)blockIdx.x * SLICE;
#pragma unroll 1
    for (int k = 0; k < SLICE_PER_LANE; ++k) {
        const long long i = i0 + k * THREADS + threadIdx.x;
        if (i >= n) break;
        const V3 b = load3(tip + (size_t)i * 3);
        if (states[i] != 0 || !finite3(b)) continue;   // selection, never arithmetic on a NaN
        if constexpr (MODE == 0) {
            acc[0] += 1.0;
            acc[1] += b.x;
            acc[2] += b.y;
            acc[3] += b.z;
        } else if constexpr (MODE == 1) {
            const V3 q = sub(b, ref);
            const double w = dot(q, q);
            acc[0] += q.x * q.x;
            acc[1] += q.x * q.y;
            acc[2] += q.x * q.z;
            acc[3] += q.x;
            acc[4] += q.y * q.y;
            acc[5] += q.y * q.z;
            acc[6] += q.y;
            acc[7] += q.z * q.z;
            acc[8] += q.z;
            acc[9] += q.x * w;
            acc[10] += q.y * w;
            acc[11] += q.z * w;
            acc[12] += w;
        } else {
            const V3 d = sub(b, ref);
            const double rho = sqrt(dot(d, d));
            const double r = rho - R;
            acc[9] += r * r;
            if (rho > 0.0) {   // a tip at the centre has no direction: it pulls nowhere
                const V3 u = {d.x / rho, d.y / rho, d.z / rho};
                acc[0] += u.x * u.x;
                acc[1] += u.x * u.y;
                acc[2] += u.x * u.z;
                acc[3] += u.y * u.y;
                acc[4] += u.y * u.z;
                acc[5] += u.z * u.z;
                acc[6] += u.x * r;
                acc[7] += u.y * r;
                acc[8] += u.z * r;
            }
        }
    }
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int o = df3d::WAVE / 2; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
        if (lane == 0) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * PART + threadIdx.x] = v;
    }
}

// lane k < count: sum k over the slices in index order, into lds
__device__ __forceinline__ void fold_slices(const double* __restrict__ part, int slices, int count, double* lds) {
    const int k = threadIdx.x;
    if (k < count) {
        double v = 0.0;
        for (int s = 0; s < slices; ++s) v += part[(size_t)s * PART + k];
        lds[k] = v;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------ the solves
// The Cholesky solve of the symmetric 3 x 3 system (xx xy xz; . yy yz; . . zz) w = rhs.  false where a pivot is at or below `floor`
// (or is no number).
__device__ __forceinline__ bool solve3(double xx, double xy, double xz, double yy, double yz, double zz, V3 rhs, double floor, V3& w) {
    if (!(xx > floor)) return false;
    const double l00 = sqrt(xx);
    const double l10 = xy / l00, l20 = xz / l00;
    const double d1 = yy - l10 * l10;
    if (!(d1 > floor)) return false;
    const double l11 = sqrt(d1);
    const double l21 = (yz - l20 * l10) / l11;
    const double d2 = zz - l20 * l20 - l21 * l21;
    if (!(d2 > floor)) return false;
    const double l22 = sqrt(d2);
    const double y0 = rhs.x / l00;
    const double y1 = (rhs.y - l10 * y0) / l11;
    const double y2 = (rhs.z - l20 * y0 - l21 * y1) / l22;
    w.z = y2 / l22;
    w.y = (y1 - l21 * w.z) / l11;
    w.x = (y0 - l10 * w.y - l20 * w.z) / l00;
    return true;
}

__device__ __forceinline__ double max2(double a, double b) { return a > b ? a : b; }

// par: count and mean of the samples; sums[0 .. 3]: the count and the sum of b
__global__ __launch_bounds__(df3d::WAVE) void ball_mean_kernel(const double* __restrict__ part, int slices, double* __restrict__ par,
                                                               double* __restrict__ sums) {
    __shared__ double s[PART];
    fold_slices(part, slices, SUMS_COUNT, s);
    if (threadIdx.x) return;
    const double n = s[0], nan = __builtin_nan("");
    par[P_COUNT] = n;
    par[P_MEAN + 0] = n > 0.0 ? s[1] / n : nan;
    par[P_MEAN + 1] = n > 0.0 ? s[2] / n : nan;
    par[P_MEAN + 2] = n > 0.0 ? s[3] / n : nan;
    for (int k = 0; k < SUMS_COUNT; ++k) sums[k] = s[k];
}

// The algebraic fit on the centred coordinates q = b - m: rows (qx, qy, qz, 1), unknowns (2 a, k), right side |q|^2.  par: centre,
// radius and status.  `radius` > 0: the known radius; the centre is then the start of the Gauss-Newton steps.
__global__ __launch_bounds__(df3d::WAVE) void ball_algebraic_kernel(const double* __restrict__ part, int slices, double radius, double pivot_min,
                                                                    double* __restrict__ par, double* __restrict__ sums) {
    __shared__ double s[PART];
    fold_slices(part, slices, SUMS_ALGEBRAIC, s);
    if (threadIdx.x) return;
    for (int k = 0; k < SUMS_ALGEBRAIC; ++k) sums[SUMS_COUNT + k] = s[k];
    const double n = par[P_COUNT], nan = __builtin_nan("");
    const V3 m = load3(par + P_MEAN);
    const bool known = radius > 0.0;
    V3 c = {nan, nan, nan};
    double R = nan;
    int status = STATUS_REFUSED;
    if (n >= 4.0) {
        // the lower triangle of the 4 x 4 Cholesky factor, row by row
        const double floor = pivot_min * max2(max2(s[0], s[4]), max2(s[7], n));
        bool ok = s[0] > floor;
        const double l00 = sqrt(s[0]);
        const double l10 = s[1] / l00, l20 = s[2] / l00, l30 = s[3] / l00;
        const double d1 = s[4] - l10 * l10;
        ok = ok && d1 > floor;
        const double l11 = sqrt(d1);
        const double l21 = (s[5] - l20 * l10) / l11, l31 = (s[6] - l30 * l10) / l11;
        const double d2 = s[7] - l20 * l20 - l21 * l21;
        ok = ok && d2 > floor;
        const double l22 = sqrt(d2);
        const double l32 = (s[8] - l30 * l20 - l31 * l21) / l22;
        const double d3 = n - l30 * l30 - l31 * l31 - l32 * l32;
        ok = ok && d3 > floor;
        const double l33 = sqrt(d3);
        const double y0 = s[9] / l00;
        const double y1 = (s[10] - l10 * y0) / l11;
        const double y2 = (s[11] - l20 * y0 - l21 * y1) / l22;
        const double y3 = (s[12] - l30 * y0 - l31 * y1 - l32 * y2) / l33;
        const double p3 = y3 / l33;
        const double p2 = (y2 - l32 * p3) / l22;
        const double p1 = (y1 - l21 * p2 - l31 * p3) / l11;
        const double p0 = (y0 - l10 * p1 - l20 * p2 - l30 * p3) / l00;
        const V3 a = {0.5 * p0, 0.5 * p1, 0.5 * p2};
        const double R2 = p3 + dot(a, a);
        if (ok && R2 > 0.0 && isfinite(R2) && finite3(a)) {
            c = {a.x + m.x, a.y + m.y, a.z + m.z};
            R = known ? radius : sqrt(R2);
            status = 0;
        }
    }
    if (status && known && n >= 3.0) {
        // three samples or a flat set have no algebraic centre; the ball lies beyond the tips as seen from the body's origin
        const double len = sqrt(dot(m, m));
        if (len > 0.0 && isfinite(len)) {
            const double f = radius / len;
            c = {m.x + m.x * f, m.y + m.y * f, m.z + m.z * f};
            R = radius;
            status = STATUS_START_BELOW;
        }
    }
    par[P_CENTER + 0] = c.x;
    par[P_CENTER + 1] = c.y;
    par[P_CENTER + 2] = c.z;
    par[P_RADIUS] = R;
    par[P_STATUS] = (double)status;
}

// One Gauss-Newton step on sum (|b - c| - R)^2 from the sums at the current centre (`step`), or the end of the fit (`last`: the sums
// are those at the final centre): ball [8] = centre, radius, rms and three zeros, info [2] = count, status.
__global__ __launch_bounds__(df3d::WAVE) void ball_step_kernel(const double* __restrict__ part, int slices, int last, double pivot_min,
                                                               double* __restrict__ par, double* __restrict__ ball, long long* __restrict__ info) {
    __shared__ double s[PART];
    fold_slices(part, slices, SUMS_STEP, s);
    if (threadIdx.x) return;
    const double nan = __builtin_nan("");
    int status = (int)par[P_STATUS];
    if (!last) {
        if (status & STATUS_REFUSED) return;
        V3 delta;
        const double floor = pivot_min * max2(max2(s[0], s[3]), s[5]);
        if (solve3(s[0], s[1], s[2], s[3], s[4], s[5], V3{s[6], s[7], s[8]}, floor, delta) && finite3(delta)) {
            par[P_CENTER + 0] += delta.x;
            par[P_CENTER + 1] += delta.y;
            par[P_CENTER + 2] += delta.z;
        } else {
            par[P_CENTER + 0] = par[P_CENTER + 1] = par[P_CENTER + 2] = par[P_RADIUS] = nan;
            par[P_STATUS] = (double)(status | STATUS_REFUSED);
        }
        return;
    }
    const bool refused = status & STATUS_REFUSED;
    const double n = par[P_COUNT];
    ball[0] = par[P_CENTER + 0];
    ball[1] = par[P_CENTER + 1];
    ball[2] = par[P_CENTER + 2];
    ball[3] = par[P_RADIUS];
    ball[4] = refused ? nan : sqrt(s[9] / n);
    ball[5] = ball[6] = ball[7] = 0.0;
    info[0] = (long long)n;
    info[1] = status;
}

// ------------------------------------------------------------------------------------------------------------------ the rotation
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__global__ __launch_bounds__(THREADS) void ball_rotation_kernel(const double* __restrict__ tip, const double* __restrict__ vel,
                                                                const int* __restrict__ states, long long T, const double* __restrict__ ball,
                                                                int min_legs, double pivot_min, double* __restrict__ omega, int* __restrict__ legs,
                                                                double* __restrict__ residual, double* __restrict__ fictive) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const V3 c = load3(ball);
    const double R = ball[3], nan = __builtin_nan("");
    const bool ball_ok = finite3(c) && isfinite(R);
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    V3 rhs = {0.0, 0.0, 0.0};
    int n = 0;
#pragma unroll
    for (int leg = 0; leg < LEGS; ++leg) {
        const size_t g = (size_t)t * LEGS + leg;
        const V3 b = load3(tip + g * 3), v = load3(vel + g * 3);
        if (states[g] != 0 || !finite3(b) || !finite3(v)) continue;   // selection, never arithmetic on a NaN
        ++n;
        const V3 r = sub(b, c);
        const double rr = dot(r, r);
        xx += rr - r.x * r.x;
        xy += -(r.x * r.y);
        xz += -(r.x * r.z);
        yy += rr - r.y * r.y;
        yz += -(r.y * r.z);
        zz += rr - r.z * r.z;
        const V3 m = cross(r, v);
        rhs = {rhs.x + m.x, rhs.y + m.y, rhs.z + m.z};
    }
    legs[t] = n;
    V3 w = {nan, nan, nan};
    bool ok = ball_ok && n >= min_legs;
    if (ok) {
        ok = solve3(xx, xy, xz, yy, yz, zz, rhs, pivot_min * (xx + yy + zz), w) && finite3(w);
        if (!ok) w = {nan, nan, nan};
    }
    double sq = 0.0;
    if (ok) {
#pragma unroll
        for (int leg = 0; leg < LEGS; ++leg) {
            const size_t g = (size_t)t * LEGS + leg;
            const V3 b = load3(tip + g * 3), v = load3(vel + g * 3);
            if (states[g] != 0 || !finite3(b) || !finite3(v)) continue;
            const V3 e = sub(v, cross(w, sub(b, c)));
            sq += dot(e, e);
        }
    }
    double* wp = omega + (size_t)t * 3;
    wp[0] = w.x;
    wp[1] = w.y;
    wp[2] = w.z;
    residual[t] = ok ? sqrt(sq / (double)n) : nan;
    // the fly stands at the body's origin, which is 0 in these coordinates: u = (o - c) / |o - c| = -c / |c|
    const double len = sqrt(dot(c, c));
    const bool moves = ok && len > 0.0;
    const V3 u = {-c.x / len, -c.y / len, -c.z / len};
    const V3 s = cross(w, V3{R * u.x, R * u.y, R * u.z});
    double* fp = fictive + (size_t)t * 3;
    fp[0] = moves ? -s.x : nan;          // forward: ex is (1, 0, 0) in body coordinates
    fp[1] = moves ? -s.y : nan;          // sideways
    fp[2] = moves ? -dot(w, u) : nan;    // yaw rate
}

// ------------------------------------------------------------------------------------------------------------------ the path
// The term of row `row` of stage STAGE at frame t.  Stage 0: yaw / fps.  Stage 1: Rot(theta_t)(forward, sideways) / fps, rows x and y,
// theta_t read from path.  A frame with a non-finite fictive component moves nothing.
template <int STAGE>
__device__ __forceinline__ double path_term(const double* __restrict__ fictive, const double* path, long long t, long long T, double fps, int row,
                                            bool& skipped) {
    skipped = false;
    if (t >= T) return 0.0;
    const V3 f = load3(fictive + (size_t)t * 3);
    if (!finite3(f)) {
        skipped = true;
        return 0.0;
    }
    if (STAGE == 0) return f.z / fps;
    double sn, cs;
    sincos(path[(size_t)t * 3 + 2], &sn, &cs);
    return (row == 0 ? cs * f.x - sn * f.y : sn * f.x + cs * f.y) / fps;
}

__global__ __launch_bounds__(THREADS) void path_zero_kernel(unsigned long long* __restrict__ skipped) {
    if (threadIdx.x == 0 && blockIdx.x == 0) skipped[0] = 0ULL;
}

// sums [rows, nb]; blockIdx.y = the row.  Stage 0 also counts the frames that move nothing.
template <int STAGE>
__global__ __launch_bounds__(THREADS) void path_blocks_kernel(const double* __restrict__ fictive, const double* path, long long T, double fps,
                                                              double* __restrict__ sums, unsigned long long* __restrict__ skipped) {
    __shared__ double lds[THREADS];
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    bool skip;
    double ex, total;
    block_scan(path_term<STAGE>(fictive, path, t, T, fps, blockIdx.y, skip), 0.0, SumOp(), lds, ex, total);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
    if (STAGE == 0) {
        const int count = __syncthreads_count(skip);
        if (threadIdx.x == 0 && count) atomicAdd(skipped, (unsigned long long)count);   // an integer: any order gives the same
    }
}

// one block per row: the row's block results -> their exclusive scan, in place, 256 at a time with a carry
__global__ __launch_bounds__(THREADS) void path_carry_kernel(double* __restrict__ sums, long long nb) {
    __shared__ double lds[THREADS];
    double* row = sums + (size_t)blockIdx.y * nb;
    double carry = 0.0;
    for (long long b0 = 0; b0 < nb; b0 += THREADS) {
        const long long b = b0 + threadIdx.x;
        double ex, chunk;
        block_scan(b < nb ? row[b] : 0.0, 0.0, SumOp(), lds, ex, chunk);
        if (b < nb) row[b] = carry + ex;
        carry += chunk;
    }
}

// path [T, 3] = (x, y, theta): stage 0 writes column 2, stage 1 columns 0 and 1 (it reads column 2 alone)
template <int STAGE>
__global__ __launch_bounds__(THREADS) void path_apply_kernel(const double* __restrict__ fictive, double* path, long long T, double fps,
                                                             const double* __restrict__ sums) {
    __shared__ double lds[THREADS];
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    bool skip;
    double ex, total;
    block_scan(path_term<STAGE>(fictive, path, t, T, fps, blockIdx.y, skip), 0.0, SumOp(), lds, ex, total);
    if (t < T) path[(size_t)t * 3 + (STAGE == 0 ? 2 : blockIdx.y)] = sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + ex;
}

// ------------------------------------------------------------------------------------------------------------------ host side
long long slices_of(long long n) { return (n + SLICE - 1) / SLICE; }

// One workspace layout serves every entry: the slice partials [slices, 16], the parameter block and the scans' block results [2, nb].
struct Layout {
    long long part, par, scan, bytes;
};

Layout layout_of(long long T) {
    Layout l;
    l.part = 0;
    l.par = l.part + round64(slices_of(LEGS * T) * PART * 8);
    l.scan = l.par + round64(P_DOUBLES * 8);
    l.bytes = l.scan + round64(2 * blocks_of(T) * 8);
    return l;
}

#define BALL_CHECK_T(T) DF3D_CHECK_ARG((T) >= 0 && (T) <= T_MAX, "T must be in [0, (2^31 - 1) / 6]")
#define BALL_CHECK_WORK(need) DF3D_CHECK_ARG(work_len_bytes >= (need), "work buffer too small (df3d_ball_work_bytes)")
#define BALL_CHECK_PIVOT(p) DF3D_CHECK_ARG((p) >= 0.0 && (p) < 1.0, "pivot_min must be in [0, 1)")

}  // namespace

extern "C" long long df3d_ball_work_bytes(long long T) { return T < 0 || T > T_MAX ? 0 : layout_of(T).bytes; }

extern "C" int df3d_ball_tips(const double* pts_dev, long long T, const double* frame_dev, const double* coxa_dev, double fps, int half_window,
                              double* tip_dev, double* vel_dev, void* stream) {
    BALL_CHECK_T(T);
    DF3D_CHECK_ARG(std::isfinite(fps) && fps > 0.0, "fps must be finite and > 0");
    DF3D_CHECK_ARG(half_window >= HALF_MIN && half_window <= HALF_MAX, "half_window must be in [1, 64]");
    if (T == 0) return DF3D_OK;
    DF3D_BUFFERS({"pts", pts_dev, T * JOINTS * 24, 8}, {"frame", frame_dev, 72, 8}, {"coxa", coxa_dev, LEGS * 24, 8},
                 {"tip", tip_dev, T * LEGS * 24, 8}, {"vel", vel_dev, T * LEGS * 24, 8});
    hipLaunchKernelGGL(ball_tips_kernel, dim3(grid_of(T * LEGS)), dim3(THREADS), 0, df3d::as_stream(stream), pts_dev, T, frame_dev, coxa_dev, fps,
                       half_window, tip_dev, vel_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_ball_fit(const double* tip_dev, const int* states_dev, long long T, int known_radius, double radius, int iterations,
                             double pivot_min, double* ball_dev, long long* info_dev, double* sums_dev, void* work_dev, long long work_len_bytes,
                             void* stream) {
    BALL_CHECK_T(T);
    DF3D_CHECK_ARG(known_radius == 0 || known_radius == 1, "known_radius must be 0 or 1");
    if (known_radius) {
        DF3D_CHECK_ARG(std::isfinite(radius) && radius > 0.0, "radius must be finite and > 0");
        DF3D_CHECK_ARG(iterations >= ITER_MIN && iterations <= ITER_MAX, "iterations must be in [1, 64]");
    }
    BALL_CHECK_PIVOT(pivot_min);
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    BALL_CHECK_WORK(l.bytes);
    DF3D_BUFFERS({"tip", tip_dev, T * LEGS * 24, 8}, {"states", states_dev, T * LEGS * 4, 4}, {"ball", ball_dev, 64, 8}, {"info", info_dev, 16, 8},
                 {"sums", sums_dev, SUMS_OUT * 8, 8}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    const long long n = LEGS * T;
    const int slices = (int)slices_of(n);
    double *part = at<double>(work_dev, l.part), *par = at<double>(work_dev, l.par);
    const dim3 grid((unsigned)slices), block(THREADS), wave(df3d::WAVE);
    hipLaunchKernelGGL(ball_sums_kernel<0>, grid, block, 0, st, tip_dev, states_dev, n, par, part);
    hipLaunchKernelGGL(ball_mean_kernel, dim3(1), wave, 0, st, part, slices, par, sums_dev);
    hipLaunchKernelGGL(ball_sums_kernel<1>, grid, block, 0, st, tip_dev, states_dev, n, par, part);
    hipLaunchKernelGGL(ball_algebraic_kernel, dim3(1), wave, 0, st, part, slices, known_radius ? radius : 0.0, pivot_min, par, sums_dev);
    for (int k = 0; k < (known_radius ? iterations : 0); ++k) {
        hipLaunchKernelGGL(ball_sums_kernel<2>, grid, block, 0, st, tip_dev, states_dev, n, par, part);
        hipLaunchKernelGGL(ball_step_kernel, dim3(1), wave, 0, st, part, slices, 0, pivot_min, par, ball_dev, info_dev);
    }
    hipLaunchKernelGGL(ball_sums_kernel<2>, grid, block, 0, st, tip_dev, states_dev, n, par, part);
    hipLaunchKernelGGL(ball_step_kernel, dim3(1), wave, 0, st, part, slices, 1, pivot_min, par, ball_dev, info_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_ball_rotation(const double* tip_dev, const double* vel_dev, const int* states_dev, long long T, const double* ball_dev,
                                  int min_legs, double pivot_min, double* omega_dev, int* legs_dev, double* residual_dev, double* fictive_dev,
                                  void* stream) {
    BALL_CHECK_T(T);
    DF3D_CHECK_ARG(min_legs >= LEGS_MIN && min_legs <= LEGS, "min_legs must be in [2, 6]");
    BALL_CHECK_PIVOT(pivot_min);
    if (T == 0) return DF3D_OK;
    DF3D_BUFFERS({"tip", tip_dev, T * LEGS * 24, 8}, {"vel", vel_dev, T * LEGS * 24, 8}, {"states", states_dev, T * LEGS * 4, 4},
                 {"ball", ball_dev, 64, 8}, {"omega", omega_dev, T * 24, 8}, {"legs", legs_dev, T * 4, 4}, {"residual", residual_dev, T * 8, 8},
                 {"fictive", fictive_dev, T * 24, 8});
    hipLaunchKernelGGL(ball_rotation_kernel, dim3(grid_of(T)), dim3(THREADS), 0, df3d::as_stream(stream), tip_dev, vel_dev, states_dev, T, ball_dev,
                       min_legs, pivot_min, omega_dev, legs_dev, residual_dev, fictive_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_ball_path(const double* fictive_dev, long long T, double fps, double* path_dev, long long* skipped_dev, void* work_dev,
                              long long work_len_bytes, void* stream) {
    BALL_CHECK_T(T);
    DF3D_CHECK_ARG(std::isfinite(fps) && fps > 0.0, "fps must be finite and > 0");
    if (T == 0) return DF3D_OK;
    const Layout l = layout_of(T);
    BALL_CHECK_WORK(l.bytes);
    DF3D_BUFFERS({"fictive", fictive_dev, T * 24, 8}, {"path", path_dev, T * 24, 8}, {"skipped", skipped_dev, 8, 8}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    double* sums = at<double>(work_dev, l.scan);
    unsigned long long* skipped = reinterpret_cast<unsigned long long*>(skipped_dev);
    const long long nb = blocks_of(T);
    const dim3 block(THREADS), one(grid_of(T), 1), two(grid_of(T), 2);
    hipLaunchKernelGGL(path_zero_kernel, dim3(1), block, 0, st, skipped);
    hipLaunchKernelGGL(path_blocks_kernel<0>, one, block, 0, st, fictive_dev, path_dev, T, fps, sums, skipped);
    hipLaunchKernelGGL(path_carry_kernel, dim3(1, 1), block, 0, st, sums, nb);
    hipLaunchKernelGGL(path_apply_kernel<0>, one, block, 0, st, fictive_dev, path_dev, T, fps, sums);
    hipLaunchKernelGGL(path_blocks_kernel<1>, two, block, 0, st, fictive_dev, path_dev, T, fps, sums, skipped);
    hipLaunchKernelGGL(path_carry_kernel, dim3(1, 2), block, 0, st, sums, nb);
    hipLaunchKernelGGL(path_apply_kernel<1>, two, block, 0, st, fictive_dev, path_dev, T, fps, sums);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
