// a3: per-(view, joint) heat-map arg-max + peak confidence.   HBM-bound, read-once.
//
// One 64-lane wavefront owns one H*W plane (64*128 = 8192 floats = 32 KiB): every iteration the wave
// reads 1 KiB contiguous (float4 per lane), four iterations are kept in flight.  Each lane scans its
// elements in increasing flat index with a strict '>' so the first occurrence wins inside the lane;
// the cross-lane butterfly keeps the larger value and, on equal values, the smaller index, which
// reproduces numpy's first-index tie-break (oracle/geometry.py:heatmap_argmax).
#include "argmax_dev.h"

extern "C" int df3d_heatmap_argmax_checked(const float* hm_dev, int n, int joints, int h, int w, float* pts_dev,
                                           float* conf_dev, int* nonfinite_planes_dev, void* stream) {
    DF3D_CHECK_ARG(n >= 0 && joints > 0 && h > 0 && w > 0, "bad shape");
    DF3D_CHECK_ARG(((h * w) & 3) == 0, "h*w must be a multiple of 4");
    if (n == 0) return DF3D_OK;
    DF3D_CHECK_ARG(hm_dev && pts_dev && conf_dev, "null pointer");
    DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(hm_dev) & 15) == 0, "heat-maps must be 16-byte aligned");
    const long long planes = (long long)n * joints;
    DF3D_CHECK_ARG(planes < (1ll << 31), "too many planes");
    const int blocks = (int)((planes + 3) / 4);
    // (row / h) computed as row * (1/h): exact for the power-of-two grids of the reference (64, 128);
    // for other sizes divide exactly instead
    const bool pow2 = ((h & (h - 1)) == 0) && ((w & (w - 1)) == 0);
    DF3D_CHECK_ARG(pow2, "h and w must be powers of two (reference heat-maps are 64 x 128)");
    hipLaunchKernelGGL(df3d::argmax_kernel<false>, dim3(blocks), dim3(256), 0, df3d::as_stream(stream), hm_dev, (int)planes,
                       h * w, w, 1.0f / (float)h, 1.0f / (float)w, pts_dev, conf_dev, nonfinite_planes_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_heatmap_argmax(const float* hm_dev, int n, int joints, int h, int w, float* pts_dev,
                                   float* conf_dev, void* stream) {
    return df3d_heatmap_argmax_checked(hm_dev, n, joints, h, w, pts_dev, conf_dev, nullptr, stream);
}
