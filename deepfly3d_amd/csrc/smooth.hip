// a6d temporal smoothing of the 2-D detections for display (the semantics are those of reference
// df3d/signal_util.py:135-160 `smooth_pose2d`, restated in float64 by tests/smooth_oracle.py).
//
// Every (camera, channel) series is filtered along T on its own: output t looks at the W samples t - W/2 .. t + W/2 - 1 of the
// edge-replicated series, takes their population variance and writes sum_k w_smooth[k] x[k] when the variance is below thr^2,
// sum_k w_keep[k] x[k] otherwise.  Both coefficient vectors are built by the host (ops.gaussian_window_taps: a Gaussian folded
// onto the window under nearest extension) and travel as kernel arguments.
//
// One 256-thread block per (camera, tile of 64 frames): the tile and its W - 1 halo frames, all nch channels wide, are staged in
// LDS once -- a tile in the interior of the recording is ONE contiguous run of (64 + W - 1) * nch doubles, so the loads are
// coalesced 8-byte lanes; only the first and last tiles clamp frame ids -- and output o of the tile reads LDS word o + k * nch for
// tap k: neighbouring lanes read neighbouring doubles, conflict-free.  64 + 19 frames x 76 channels = 50.5 KB, three blocks per CU.
// The window is read twice at most (mean; then deviations and the weighted sum in one sweep); at W = 20, the only width the
// package uses, it is read once into registers.  ~4 float64 operations per tap: the pass is bound by the float64 vector rate as
// much as by memory (DESIGN.md section 11 has the numbers).
#include <cfloat>

#include "common.h"

namespace {

constexpr int TILE = 64;       // frames per block; tests/test_gpu_smooth.py sweeps T around its multiples
constexpr int THREADS = 256;
constexpr int MAX_W = 64;
constexpr int MAX_NCH = 128;
constexpr int MAX_C = 8;

struct Taps {
    double c[MAX_W];
};

// One output from its window col[0], col[stride], ..., W taps.  The variance is mean((x - mean)^2), the mean a left-to-right sum
// times 1 / W.  A window that holds a NaN or an infinity has a NaN variance: the test is false and the keep taps apply; taps that
// are exactly zero are skipped there (a uniform branch), so that the reference's one-tap keep filter returns the centre sample
// itself whatever its neighbours hold.  That filter -- a single non-zero tap, keep_tap >= 0 with weight keep_w -- is one LDS read
// and one multiply; only a keep filter of several taps walks the window again.
template <int WT>
__device__ __forceinline__ double smooth_one(const Taps& ws, const Taps& wk, const double* col, int stride, int w_rt, double inv_w,
                                             double thr2, int keep_tap, double keep_w) {
    const int W = WT ? WT : w_rt;
    double x[WT ? WT : 1];
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const double v = col[k * stride];
        if (WT) x[k] = v;
        sum += v;
    }
    const double mean = sum * inv_w;
    double ss = 0.0, acc = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const double v = WT ? x[k] : col[k * stride];
        const double d = v - mean;
        ss = fma(d, d, ss);
        acc = fma(ws.c[k], v, acc);
    }
    if (ss * inv_w < thr2) return acc;
    if (keep_tap >= 0) return keep_w * col[keep_tap * stride];
    acc = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if (wk.c[k] != 0.0) acc = fma(wk.c[k], WT ? x[k] : col[k * stride], acc);
    }
    return acc;
}

template <int WT>
__global__ __launch_bounds__(THREADS) void smooth_kernel(Taps ws, Taps wk, const double* __restrict__ pts, double* __restrict__ out,
                                                         long long T, int nch, int w_rt, double inv_w, double thr2, int keep_tap,
                                                         double keep_w) {
    extern __shared__ double tile[];   // [TILE + W - 1][nch]
    const int W = WT ? WT : w_rt;
    const long long f0 = (long long)blockIdx.x * TILE;
    const size_t cam = (size_t)blockIdx.y * (size_t)T * nch;
    const double* src = pts + cam;
    const int rows = TILE + W - 1;
    const int n = rows * nch;
    const long long first = f0 - W / 2;
    if (first >= 0 && first + rows <= T) {
        const double* run = src + first * nch;
        for (int e = threadIdx.x; e < n; e += THREADS) tile[e] = run[e];
    } else {   // the recording's edges: frames before 0 read frame 0, frames after T - 1 read frame T - 1
        for (int e = threadIdx.x; e < n; e += THREADS) {
            const int r = e / nch, ch = e - r * nch;
            long long f = first + r;
            f = f < 0 ? 0 : (f > T - 1 ? T - 1 : f);
            tile[e] = src[f * nch + ch];
        }
    }
    __syncthreads();
    const long long left = T - f0;
    const int live = (int)(left < TILE ? left : TILE) * nch;
    double* dst = out + cam + f0 * nch;
    for (int o = threadIdx.x; o < live; o += THREADS) dst[o] = smooth_one<WT>(ws, wk, tile + o, nch, w_rt, inv_w, thr2, keep_tap, keep_w);
}

template <int WT>
int launch(const Taps& ws, const Taps& wk, const double* pts, double* out, int C, long long T, int nch, int window, double thr2,
           hipStream_t stream) {
    const size_t lds = sizeof(double) * (size_t)(TILE + window - 1) * nch;   // at most 127 * 128 * 8 = 130 048 bytes
    // Tiles beyond 64 KB (nch > 98 at W = 20; never the package's own 76 channels) need the limit raised.  The attribute belongs to
    // the CURRENT device, and a process may drive several, so it is set on every such launch rather than once per process
    if (lds > 64 * 1024)
        DF3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(smooth_kernel<WT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long tiles = (T + TILE - 1) / TILE;
    int keep_tap = -1, keep_taps = 0;
    for (int k = 0; k < window; ++k) {
        if (wk.c[k] != 0.0) {
            keep_tap = k;
            ++keep_taps;
        }
    }
    if (keep_taps != 1) keep_tap = -1;
    hipLaunchKernelGGL(smooth_kernel<WT>, dim3((unsigned)tiles, (unsigned)C), dim3(THREADS), lds, stream, ws, wk, pts, out, T, nch, window,
                       1.0 / window, thr2, keep_tap, keep_tap >= 0 ? wk.c[keep_tap] : 0.0);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

}  // namespace

extern "C" int df3d_smooth_pose2d(const double* pts_dev, int C, long long T, int nch, int window, double std_thr, const double* w_smooth_host,
                                  const double* w_keep_host, double* out_dev, void* stream) {
    DF3D_CHECK_ARG(C >= 1 && C <= MAX_C, "C must be in [1, 8]");
    DF3D_CHECK_ARG(nch >= 1 && nch <= MAX_NCH, "nch must be in [1, 128]");
    DF3D_CHECK_ARG(window >= 2 && window <= MAX_W && window % 2 == 0, "window must be even and in [2, 64]");
    DF3D_CHECK_ARG(std_thr >= 0.0, "std_thr must be >= 0 and not NaN");
    DF3D_CHECK_ARG(T >= 0 && T <= (long long)TILE * 0x7fffffffLL, "T must be >= 0 (and at most 64 * (2^31 - 1))");
    DF3D_CHECK_ARG(w_smooth_host && w_keep_host, "null coefficient pointer");
    Taps ws, wk;
    memset(&ws, 0, sizeof(ws));
    memset(&wk, 0, sizeof(wk));
    for (int k = 0; k < window; ++k) {
        DF3D_CHECK_ARG(std::isfinite(w_smooth_host[k]) && std::isfinite(w_keep_host[k]), "coefficients must be finite");
        ws.c[k] = w_smooth_host[k];
        wk.c[k] = w_keep_host[k];
    }
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(pts_dev && out_dev, "null pointer");
    const size_t count = (size_t)C * (size_t)T * nch;
    DF3D_CHECK_ARG(out_dev + count <= pts_dev || pts_dev + count <= out_dev, "out must not alias pts (a tile reads its neighbours' frames)");
    // the test is std < thr, taken as variance < thr^2: the two differ only where std is within an ulp of thr.  A positive thr
    // below ~1.5e-154 squares to 0, which would keep a constant window (std 0) that the reference smooths: the smallest positive
    // double stands in, below every non-zero variance such a thr could admit
    double thr2 = std_thr * std_thr;
    if (thr2 == 0.0 && std_thr > 0.0) thr2 = DBL_TRUE_MIN;
    if (window == 20) return launch<20>(ws, wk, pts_dev, out_dev, C, T, nch, window, thr2, df3d::as_stream(stream));
    return launch<0>(ws, wk, pts_dev, out_dev, C, T, nch, window, thr2, df3d::as_stream(stream));
}
