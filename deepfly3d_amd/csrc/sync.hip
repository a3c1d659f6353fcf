// a23 per-camera frame lags from epipolar consistency (the model is this project's own specification, stated in
// numpy / int64 by tests/sync_oracle.py).  Cameras a < b of a pair, lag d in [-D, D]: camera a's frame t is paired with camera b's frame
// t + d for every joint, the sample's squared Sampson distance against F_ab is truncated at tau^2 and rounded once to an int64 cost in
// units of 2^-10 px^2, and the costs and counts are summed per window of W of camera a's frames.  Everything after that rounding is
// integer arithmetic, so no sum depends on its order and the tables are compared exactly.  No atomics: two runs give the same bits.
//
// pair_costs_kernel: a workgroup owns (window, group of LAGS consecutive lags, pair).  Its four waves walk the window in chunks of
//   FRAMES = 4 frames, a wave a frame, a lane a joint: the lane reads camera a's detection and forms l = F x_a once, then meets camera b's
//   frames t + d for all lags of the group, adding into LAGS cost / count registers (the lag loop is unrolled: static register indices).
//   Camera a's window is read once for all lags of the group; the groups of a window are what fills the device (one group of 17 lags
//   leaves 24 workgroups per 1 000 frames of the fly rig: 354 us of kernel time there against 68 us with groups of 3).  The lanes' sums are added
//   inside each wave by an xor butterfly and across the four waves through LDS.
// paths_kernel: a workgroup per pair, a lane per lag state: the exact Viterbi over the windows on int64 (the two rows of values in LDS,
//   the predecessors as bytes in the caller's work buffer), the backtrack by lane 0, then the margins, a lane a window.
// apply_kernel: the gather out[c, t, j] = in[c, t + lag_cam[c, t / W], j], zero where that frame does not exist.
#include <cmath>
#include <cstdint>

#include "buffer_check.h"

// Built with -ffp-contract=off (build.py): the Sampson distance is the oracle's multiplies and adds one by one.

namespace {

constexpr int MAX_CAM = 8;
constexpr int MAX_J = 64;
constexpr int MAX_PAIR = MAX_CAM * (MAX_CAM - 1) / 2;
constexpr int MAX_D = 64;
constexpr int MAX_STATES = 2 * MAX_D + 1;
constexpr int MAX_T = 1 << 20;
constexpr double MAX_TAU = 4096.0;                 // tau^2 2^10 = 2^34: T J <= 2^26 samples sum below 2^60
constexpr long long MAX_SWITCH = 1LL << 34;        // kappa q: times 2 D <= 2^7 per window, 2^20 windows: below 2^61
constexpr double COST_SCALE = 1024.0;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / df3d::WAVE;
constexpr int FRAMES = WAVES;    // frames of a workgroup's chunk: a wave each
constexpr int LAGS = 3;          // lags of a workgroup: 6 groups at the default 17 lags, 144 workgroups per 1 000 frames of the fly rig

struct Pairs {
    double F[MAX_PAIR][9];
    int a[MAX_PAIR], b[MAX_PAIR];
};

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 1; o < df3d::WAVE; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(THREADS) void pair_costs_kernel(Pairs pairs, const double* __restrict__ pts, int T, int J, int D, int W, double tau2,
                                                             long long* __restrict__ cost, long long* __restrict__ count) {
    __shared__ long long part[WAVES][LAGS][2];
    const int tid = threadIdx.x, lane = tid % df3d::WAVE, wave = tid / df3d::WAVE;
    const int w = blockIdx.x, pair = blockIdx.z, nW = gridDim.x, nL = 2 * D + 1;
    const int s0 = blockIdx.y * LAGS;   // the group's first state; state s is lag s - D
    const double* F = pairs.F[pair];
    const double f0 = F[0], f1 = F[1], f2 = F[2], f3 = F[3], f4 = F[4], f5 = F[5], f6 = F[6], f7 = F[7], f8 = F[8];
    const size_t TJ = (size_t)T * J;
    const double* pa = pts + (size_t)pairs.a[pair] * TJ * 2;
    const double* pb = pts + (size_t)pairs.b[pair] * TJ * 2;
    const int t0 = w * W, t1 = T - t0 < W ? T : t0 + W;   // t0 < T <= 2^20, W >= 1: no overflow

    long long c[LAGS], n[LAGS];
#pragma unroll
    for (int g = 0; g < LAGS; ++g) c[g] = 0, n[g] = 0;
    for (int t = t0 + wave; t < t1; t += FRAMES) {
        if (lane >= J) continue;
        const double ya = pa[((size_t)t * J + lane) * 2], xa = pa[((size_t)t * J + lane) * 2 + 1];   // (row, col): x = (col, row, 1)
        if (xa == 0.0 || ya == 0.0) continue;
        const double l0 = f0 * xa + f1 * ya + f2;
        const double l1 = f3 * xa + f4 * ya + f5;
        const double l2 = f6 * xa + f7 * ya + f8;
        const double ll = l0 * l0 + l1 * l1;
#pragma unroll
        for (int g = 0; g < LAGS; ++g) {
            const int tb = t + (s0 + g - D);
            if (s0 + g >= nL || tb < 0 || tb >= T) continue;
            const double yb = pb[((size_t)tb * J + lane) * 2], xb = pb[((size_t)tb * J + lane) * 2 + 1];
            if (xb == 0.0 || yb == 0.0) continue;
            const double m0 = f0 * xb + f3 * yb + f6;
            const double m1 = f1 * xb + f4 * yb + f7;
            const double s = xb * l0 + yb * l1 + l2;
            const double den = ll + m0 * m0 + m1 * m1;
            if (den == 0.0) continue;
            const double e = s * s / den;
            const double m = e < tau2 ? e : tau2;   // a NaN costs tau^2
            c[g] += (long long)floor(m * COST_SCALE + 0.5);
            n[g] += 1;
        }
    }
#pragma unroll
    for (int g = 0; g < LAGS; ++g) {
        const long long cs = wave_sum(c[g]), ns = wave_sum(n[g]);
        if (lane == 0) part[wave][g][0] = cs, part[wave][g][1] = ns;
    }
    __syncthreads();
    if (tid < LAGS && s0 + tid < nL) {
        long long cs = 0, ns = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) cs += part[v][tid][0], ns += part[v][tid][1];
        const size_t o = ((size_t)pair * nW + w) * nL + s0 + tid;
        cost[o] = cs;
        count[o] = ns;
    }
}

// the r-th lag in the order of the tie rule, the smaller (|d|, d) first: 0, -1, 1, -2, 2, ...
__device__ __forceinline__ int lag_of_rank(int r) { return r == 0 ? 0 : (r & 1 ? -((r + 1) / 2) : r / 2); }

__global__ __launch_bounds__(THREADS) void paths_kernel(const long long* __restrict__ cost, const long long* __restrict__ count, int nW, int D,
                                                        long long kq, long long min_count, int* __restrict__ lag, long long* __restrict__ path_cost,
                                                        double* __restrict__ margin, unsigned char* __restrict__ back) {
    __shared__ long long V[2][MAX_STATES];
    __shared__ int last;
    const int tid = threadIdx.x, pair = blockIdx.x, nL = 2 * D + 1;
    const long long* cp = cost + (size_t)pair * nW * nL;
    const long long* np = count + (size_t)pair * nW * nL;
    unsigned char* bp = back + (size_t)pair * nW * nL;
    int* lp = lag + (size_t)pair * nW;

    if (tid < nL) V[0][tid] = cp[tid];
    __syncthreads();
    for (int w = 1; w < nW; ++w) {
        const long long* prev = V[(w - 1) & 1];
        if (tid < nL) {
            long long best = 0;
            int from = 0;
            for (int r = 0; r < nL; ++r) {
                const int p = lag_of_rank(r) + D;
                const int jump = p > tid ? p - tid : tid - p;
                const long long v = prev[p] + kq * jump;
                if (r == 0 || v < best) best = v, from = p;
            }
            V[w & 1][tid] = cp[(size_t)w * nL + tid] + best;
            bp[(size_t)w * nL + tid] = (unsigned char)from;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const long long* fin = V[(nW - 1) & 1];
        long long best = 0;
        int at = 0;
        for (int r = 0; r < nL; ++r) {
            const int p = lag_of_rank(r) + D;
            if (r == 0 || fin[p] < best) best = fin[p], at = p;
        }
        path_cost[pair] = best;
        last = at;
    }
    __syncthreads();
    __threadfence_block();
    if (tid == 0) {
        int s = last;
        for (int w = nW - 1; w >= 0; --w) {
            lp[w] = s - D;
            if (w > 0) s = bp[(size_t)w * nL + s];   // written by this workgroup before the barriers above
        }
    }
    __syncthreads();
    for (int w = tid; w < nW; w += THREADS) {
        const int s = lp[w] + D;
        const long long* cw = cp + (size_t)w * nL;
        const long long* nw = np + (size_t)w * nL;
        double m = __builtin_nan("");
        if (nw[s] >= min_count && nw[s] > 0) {
            const double here = (double)cw[s] / (double)nw[s] / COST_SCALE;
            double other = __builtin_inf();
            for (int k = 0; k < nL; ++k)
                if (k != s && nw[k] > 0) {
                    const double v = (double)cw[k] / (double)nw[k] / COST_SCALE;
                    if (v < other) other = v;
                }
            m = other - here;
        }
        margin[(size_t)pair * nW + w] = m;
    }
}

__global__ __launch_bounds__(THREADS) void apply_kernel(const double* __restrict__ in, const int* __restrict__ lag_cam, int T, int J, int W, int nW,
                                                        long long total, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;   // over [C, T, J]
    if (i >= total) return;
    const long long TJ = (long long)T * J;
    const int c = (int)(i / TJ), j = (int)(i % J);
    const long long t = i % TJ / J;
    const long long src = t + lag_cam[(size_t)c * nW + t / W];
    double r = 0.0, cl = 0.0;
    if (src >= 0 && src < T) {
        const size_t k = (((size_t)c * T + src) * J + j) * 2;
        r = in[k], cl = in[k + 1];
    }
    out[i * 2] = r;
    out[i * 2 + 1] = cl;
}

// ------------------------------------------------------------------------------------------------------------------ host side
long long windows_of(int T, int W) { return ((long long)T + W - 1) / W; }

}  // namespace

#define DF3D_SYNC_SHAPE()                                                          \
    DF3D_CHECK_ARG(ncam >= 1 && ncam <= MAX_CAM, "ncam must be in [1, 8]");        \
    DF3D_CHECK_ARG(J >= 1 && J <= MAX_J, "J must be in [1, 64]");                  \
    DF3D_CHECK_ARG(T >= 0 && T <= MAX_T, "T must be in [0, 1048576]");             \
    DF3D_CHECK_ARG(W >= 1, "window must be >= 1")

#define DF3D_SYNC_TABLE()                                                          \
    DF3D_CHECK_ARG(npair >= 0 && npair <= MAX_PAIR, "npair must be in [0, 28]");   \
    DF3D_CHECK_ARG(D >= 0 && D <= MAX_D, "max_lag must be in [0, 64]")

extern "C" long long df3d_sync_work_bytes(int npair, long long nW, int D) {
    if (npair < 0 || npair > MAX_PAIR || nW < 0 || nW > MAX_T || D < 0 || D > MAX_D) return 0;
    const long long b = (long long)npair * nW * (2 * D + 1);
    return (b + 63) / 64 * 64 + 64;
}

extern "C" int df3d_sync_pair_costs(const double* F_host, const int* pairs_host, int npair, const double* pts_px_dev, int ncam, int T, int J, int D,
                                    int W, double tau, long long* cost_dev, long long* count_dev, void* stream) {
    DF3D_SYNC_SHAPE();
    DF3D_SYNC_TABLE();
    DF3D_CHECK_ARG(tau >= 0.0 && tau <= MAX_TAU, "tau must be in [0, 4096] and not NaN");
    if (npair == 0 || T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(F_host, "null pointer: F_host");
    DF3D_CHECK_ARG(pairs_host, "null pointer: pairs_host");
    Pairs pairs;
    memset(&pairs, 0, sizeof(pairs));
    for (int p = 0; p < npair; ++p) {
        const int a = pairs_host[2 * p], b = pairs_host[2 * p + 1];
        DF3D_CHECK_ARG(a >= 0 && a < b && b < ncam, "a pair must hold two cameras 0 <= a < b < ncam");
        pairs.a[p] = a, pairs.b[p] = b;
        memcpy(pairs.F[p], F_host + 9 * p, sizeof(double) * 9);
    }
    const long long nW = windows_of(T, W), nL = 2 * D + 1, table = (long long)npair * nW * nL * 8;
    DF3D_BUFFERS({"pts_px", pts_px_dev, (long long)ncam * T * J * 16, 8}, {"cost", cost_dev, table, 8}, {"count", count_dev, table, 8});
    hipLaunchKernelGGL(pair_costs_kernel, dim3((unsigned)nW, (unsigned)((nL + LAGS - 1) / LAGS), (unsigned)npair), dim3(THREADS), 0,
                       df3d::as_stream(stream), pairs, pts_px_dev, T, J, D, W, tau * tau, cost_dev, count_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_sync_paths(const long long* cost_dev, const long long* count_dev, int npair, long long nW, int D, long long switch_q,
                               long long min_count, int* lag_dev, long long* path_cost_dev, double* margin_dev, void* work_dev,
                               long long work_bytes, void* stream) {
    DF3D_SYNC_TABLE();
    DF3D_CHECK_ARG(nW >= 0 && nW <= MAX_T, "the number of windows must be in [0, 1048576]");
    DF3D_CHECK_ARG(switch_q >= 0 && switch_q <= MAX_SWITCH, "the switch cost must be in [0, 2^34] (2^-10 px^2)");
    DF3D_CHECK_ARG(min_count >= 0, "min_count must be >= 0");
    if (npair == 0 || nW == 0) return DF3D_OK;
    const long long need = df3d_sync_work_bytes(npair, nW, D), nL = 2 * D + 1, table = (long long)npair * nW * nL * 8;
    DF3D_CHECK_ARG(work_bytes >= need, "work buffer too small (df3d_sync_work_bytes)");
    DF3D_BUFFERS({"cost", cost_dev, table, 8}, {"count", count_dev, table, 8}, {"lag", lag_dev, (long long)npair * nW * 4, 4},
                 {"path_cost", path_cost_dev, (long long)npair * 8, 8}, {"margin", margin_dev, (long long)npair * nW * 8, 8},
                 {"work", work_dev, need, 1});
    hipLaunchKernelGGL(paths_kernel, dim3((unsigned)npair), dim3(THREADS), 0, df3d::as_stream(stream), cost_dev, count_dev, (int)nW, D, switch_q,
                       min_count, lag_dev, path_cost_dev, margin_dev, static_cast<unsigned char*>(work_dev));
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_sync_apply(const double* pts_px_dev, const int* lag_cam_dev, int ncam, int T, int J, int W, double* out_dev, void* stream) {
    DF3D_SYNC_SHAPE();
    if (T == 0) return DF3D_OK;
    const long long nW = windows_of(T, W), total = (long long)ncam * T * J;
    DF3D_BUFFERS({"pts_px", pts_px_dev, total * 16, 8}, {"lag_cam", lag_cam_dev, (long long)ncam * nW * 4, 4}, {"out", out_dev, total * 16, 8});
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, df3d::as_stream(stream), pts_px_dev,
                       lag_cam_dev, T, J, W, (int)nW, total, out_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
