// a6c per-joint reprojection errors of the 2-D detections and the per-frame "suspect joint" masks (the
// model is this project's own specification, restated in float64 by tests/reproj_oracle.py).
//
// One wave per frame, four frames per 256-thread block: lane j < J owns joint j of the frame.  The lane reads its detection in
// every camera (one 16-byte load per camera; the wave's loads of one camera are J * 16 contiguous bytes), keeps them in
// registers, counts the views (both coordinates non-zero, the rule of DF3D_DLT_ADD_VIEW), projects X[t, j] through each view
// and writes e[c, t, j] for every camera (0 for non-views), max_c e and, from lane 0, the wave ballot of "max_c e > thr[j]" as
// the frame's 64-bit mask.  Memory-bound float64: ~4.3 KB read and ~2.4 KB written per frame of 7 cameras x 38 joints; the
// lanes past J (26 of 64 at J = 38) idle, which costs no bandwidth.  P (8 x 12) and thr (64) travel as kernel arguments.
#include "geometry_dev.h"

namespace {

using df3d::CamP;
using df3d::MAX_CAM;

constexpr int MAX_J = 64;
constexpr int FRAMES_PER_BLOCK = 4;

struct Thr {
    double t[MAX_J];
};

__global__ __launch_bounds__(256) void reproj_kernel(CamP cams, Thr thr, const double* __restrict__ pts, const double* __restrict__ X,
                                                     int ncam, int T, int J, double* __restrict__ err, double* __restrict__ jmax,
                                                     long long* __restrict__ mask) {
    const int lane = threadIdx.x % df3d::WAVE;
    const int t = blockIdx.x * FRAMES_PER_BLOCK + threadIdx.x / df3d::WAVE;
    if (t >= T) return;   // uniform over the wave: the ballot below sees every lane of a live frame
    const bool live = lane < J;
    const size_t TJ = (size_t)T * J;
    const size_t tj = (size_t)t * J + lane;

    double row[MAX_CAM], col[MAX_CAM];
    int nviews = 0;
#pragma unroll
    for (int c = 0; c < MAX_CAM; ++c) {
        row[c] = 0.0;
        col[c] = 0.0;
        if (live && c < ncam) {
            const double2 rc = *reinterpret_cast<const double2*>(pts + ((size_t)c * TJ + tj) * 2);
            row[c] = rc.x;
            col[c] = rc.y;
            nviews += (rc.x != 0.0 && rc.y != 0.0) ? 1 : 0;
        }
    }
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (live && nviews >= 2) {
        x0 = X[tj * 3 + 0];
        x1 = X[tj * 3 + 1];
        x2 = X[tj * 3 + 2];
    }
    double m = 0.0;
#pragma unroll
    for (int c = 0; c < MAX_CAM; ++c) {
        if (live && c < ncam) {
            double e = 0.0;
            if (nviews >= 2 && row[c] != 0.0 && col[c] != 0.0) {
                const double* P = cams.p[c];
                const double u = P[0] * x0 + P[1] * x1 + P[2] * x2 + P[3];
                const double v = P[4] * x0 + P[5] * x1 + P[6] * x2 + P[7];
                const double w = P[8] * x0 + P[9] * x1 + P[10] * x2 + P[11];
                const double du = u / w - col[c], dv = v / w - row[c];   // x = col_px, y = row_px, as in triangulate_kernel
                e = sqrt(du * du + dv * dv);
                if (!(w > 0.0) || !isfinite(e)) e = __builtin_inf();   // behind the camera, or degenerate: always suspect
            }
            err[(size_t)c * TJ + tj] = e;
            m = fmax(m, e);
        }
    }
    if (live && jmax) jmax[tj] = m;
    const unsigned long long bits = __ballot(live && m > thr.t[lane]);
    if (lane == 0) mask[t] = (long long)bits;
}

}  // namespace

extern "C" int df3d_reproj_errors(const double* P_host, const double* pts_px_dev, const double* X_dev, int ncam, int T, int J,
                                  const double* thr_host, double* err_dev, double* jmax_dev, long long* mask_dev, void* stream) {
    DF3D_CHECK_ARG(ncam >= 1 && ncam <= MAX_CAM, "ncam must be in [1, 8]");
    DF3D_CHECK_ARG(J >= 1 && J <= MAX_J, "J must be in [1, 64] (the frame mask is 64 bits wide)");
    DF3D_CHECK_ARG(T >= 0, "T must be >= 0");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(P_host && pts_px_dev && X_dev && thr_host && err_dev && mask_dev, "null pointer");
    Thr thr;
    for (int j = 0; j < MAX_J; ++j) thr.t[j] = 0.0;
    for (int j = 0; j < J; ++j) {
        DF3D_CHECK_ARG(thr_host[j] >= 0.0, "thresholds must be >= 0 and not NaN (+inf disables a joint)");
        thr.t[j] = thr_host[j];
    }
    CamP cams;
    memset(&cams, 0, sizeof(cams));
    memcpy(cams.p, P_host, sizeof(double) * 12 * ncam);
    const int blocks = (T + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
    hipLaunchKernelGGL(reproj_kernel, dim3(blocks), dim3(FRAMES_PER_BLOCK * df3d::WAVE), 0, df3d::as_stream(stream), cams, thr, pts_px_dev,
                       X_dev, ncam, T, J, err_dev, jmax_dev, mask_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
