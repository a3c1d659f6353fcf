// a4 (19 -> 38 joint re-layout) and a6 (multi-view DLT triangulation), float64.
//
// Triangulation: one thread per (frame, joint).  The thread accumulates the 4x4 normal matrix
// M = A^T A of the DLT system (rows x*P2 - P0, y*P2 - P1 of every camera that sees the joint) in
// registers, diagonalises it with cyclic Jacobi rotations (fully unrolled, no scratch) and returns
// the eigenvector of the smallest eigenvalue = the last right-singular vector of A
// (oracle/geometry.py:triangulate_dlt).  The DLT and the re-layout rule live in geometry_dev.h, shared
// with the pictorial-structures proposals (pictorial.hip).  M is pre-scaled by 1/trace so the
// rotations work on O(1) numbers; scaling does not move eigenvectors.  Latency-bound: 5 KB/frame.
#include "geometry_dev.h"

namespace {

using df3d::CamP;
using df3d::MAX_CAM;
using df3d::jacobi_rotate;

__global__ __launch_bounds__(256) void triangulate_kernel(CamP cams, const double* __restrict__ pts, int ncam,
                                                          long long TJ, double row_scale, double col_scale,
                                                          double* __restrict__ X) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= TJ) return;

    double a[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[i][j] = 0.0;

    int nviews = 0;
    for (int c = 0; c < ncam; ++c) {
        const double2 rc = *reinterpret_cast<const double2*>(pts + ((size_t)c * TJ + idx) * 2);
        DF3D_DLT_ADD_VIEW(a, nviews, cams.p[c], rc.x * row_scale, rc.y * col_scale);
    }
    double out0 = 0.0, out1 = 0.0, out2 = 0.0;
    DF3D_DLT_SOLVE(a, nviews, out0, out1, out2);
    X[idx * 3 + 0] = out0;
    X[idx * 3 + 1] = out1;
    X[idx * 3 + 2] = out2;
}

struct Order {
    int o[7];
};

// out[7, T, 38, 2] from pts19[7, T, 19, 2]; one thread per output (cam, t, joint)
__global__ __launch_bounds__(256) void relayout_kernel(const float* __restrict__ in, Order ord, int T,
                                                       double* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = 7ll * T * 38;
    if (idx >= total) return;
    const int j = (int)(idx % 38);
    const long long ct = idx / 38;
    const int t = (int)(ct % T);
    const int cam = (int)(ct / T);
    // position of this physical camera in the ordering (ordering is a permutation of 0..6)
    int pos = -1;
#pragma unroll
    for (int k = 0; k < 7; ++k)
        if (ord.o[k] == cam) pos = k;
    double row = 0.0, col = 0.0;
    bool left;
    const int src = df3d::relayout_source(pos, j, &left);
    if (src >= 0) {
        const float2 p = *reinterpret_cast<const float2*>(in + (((size_t)cam * T + t) * 19 + src) * 2);
        row = (double)p.x;
        col = (double)p.y;
    }
    if (left) col = 1.0 - col;  // un-flip: applied to ALL 38 joints of the three left-side cameras
    out[idx * 2 + 0] = row;
    out[idx * 2 + 1] = col;
}

}  // namespace

static int triangulate_impl(const double* P_dev_or_host, const double* pts_px_dev, double row_scale, double col_scale,
                            int ncam, int T, int J, double* X_dev, void* stream) {
    DF3D_CHECK_ARG(ncam >= 1 && ncam <= MAX_CAM, "ncam must be in [1, 8]");
    DF3D_CHECK_ARG(T >= 0 && J > 0, "bad shape");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(P_dev_or_host && pts_px_dev && X_dev, "null pointer");
    // the 7 x 12 projection entries travel as a kernel argument (scalar registers / constant loads)
    CamP cams;
    memset(&cams, 0, sizeof(cams));
    hipPointerAttribute_t attr;
    bool on_device = false;
    if (hipPointerGetAttributes(&attr, P_dev_or_host) == hipSuccess)
        on_device = (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
    else
        (void)hipGetLastError();
    if (on_device) {
        DF3D_HIP(hipMemcpyAsync(cams.p, P_dev_or_host, sizeof(double) * 12 * ncam, hipMemcpyDeviceToHost,
                                df3d::as_stream(stream)));
        DF3D_HIP(hipStreamSynchronize(df3d::as_stream(stream)));
    } else {
        memcpy(cams.p, P_dev_or_host, sizeof(double) * 12 * ncam);
    }
    const long long TJ = (long long)T * J;
    const int blocks = (int)((TJ + 255) / 256);
    hipLaunchKernelGGL(triangulate_kernel, dim3(blocks), dim3(256), 0, df3d::as_stream(stream), cams, pts_px_dev,
                       ncam, TJ, row_scale, col_scale, X_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_triangulate(const double* P, const double* pts_px_dev, int ncam, int T, int J, double* X_dev,
                                void* stream) {
    return triangulate_impl(P, pts_px_dev, 1.0, 1.0, ncam, T, J, X_dev, stream);
}

extern "C" int df3d_triangulate_scaled(const double* P, const double* pts_norm_dev, double row_scale, double col_scale,
                                       int ncam, int T, int J, double* X_dev, void* stream) {
    DF3D_CHECK_ARG(row_scale > 0 && col_scale > 0, "scales must be positive");
    return triangulate_impl(P, pts_norm_dev, row_scale, col_scale, ncam, T, J, X_dev, stream);
}

extern "C" int df3d_relayout_19_to_38(const float* pts19_dev, const int* ordering_host, int T, double* out_dev,
                                      void* stream) {
    DF3D_CHECK_ARG(T >= 0, "bad T");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(pts19_dev && ordering_host && out_dev, "null pointer");
    Order ord;
    int seen = 0;
    for (int k = 0; k < 7; ++k) {
        DF3D_CHECK_ARG(ordering_host[k] >= 0 && ordering_host[k] < 7, "camera ordering entries must be in [0, 6]");
        seen |= 1 << ordering_host[k];
        ord.o[k] = ordering_host[k];
    }
    DF3D_CHECK_ARG(seen == 0x7f, "camera ordering must be a permutation of 0..6");
    const long long total = 7ll * T * 38;
    const int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(relayout_kernel, dim3(blocks), dim3(256), 0, df3d::as_stream(stream), pts19_dev, ord, T,
                       out_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
