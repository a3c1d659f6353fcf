// Opt-in sub-pixel localisation of heat-map peaks: the arg-max kernel of argmax.hip and the peaks kernel of
// pictorial.hip, instantiated with the refinement of subpixel_dev.h after their reductions.  Cell, confidence / peak values, peak order
// and the non-finite counter are those of the plain entries (shared code, argmax_dev.h and peaks_dev.h); only the points differ, by at
// most half a cell per axis.
//
// build.py compiles this file with -ffp-contract=off: the float64 rule is compared bit for bit with tests/subpixel_oracle.py.
#include "argmax_dev.h"
#include "peaks_dev.h"

extern "C" int df3d_heatmap_argmax_subpixel(const float* hm_dev, int n, int joints, int h, int w, float* pts_dev, float* conf_dev,
                                            int* nonfinite_planes_dev, void* stream) {
    // the checks of df3d_heatmap_argmax_checked
    DF3D_CHECK_ARG(n >= 0 && joints > 0 && h > 0 && w > 0, "bad shape");
    DF3D_CHECK_ARG(((h * w) & 3) == 0, "h*w must be a multiple of 4");
    if (n == 0) return DF3D_OK;
    DF3D_CHECK_ARG(hm_dev && pts_dev && conf_dev, "null pointer");
    DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(hm_dev) & 15) == 0, "heat-maps must be 16-byte aligned");
    const long long planes = (long long)n * joints;
    DF3D_CHECK_ARG(planes < (1ll << 31), "too many planes");
    const int blocks = (int)((planes + 3) / 4);
    const bool pow2 = ((h & (h - 1)) == 0) && ((w & (w - 1)) == 0);
    DF3D_CHECK_ARG(pow2, "h and w must be powers of two (reference heat-maps are 64 x 128)");
    hipLaunchKernelGGL(df3d::argmax_kernel<true>, dim3(blocks), dim3(256), 0, df3d::as_stream(stream), hm_dev, (int)planes, h * w, w,
                       1.0f / (float)h, 1.0f / (float)w, pts_dev, conf_dev, nonfinite_planes_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_heatmap_peaks_subpixel(const float* hm_dev, int n, int joints, int h, int w, int k, int* count_dev, float* pts_dev,
                                           float* val_dev, void* stream) {
    // the checks of df3d_heatmap_peaks
    DF3D_CHECK_ARG(n >= 0 && joints > 0 && h > 0 && w > 0, "bad shape");
    DF3D_CHECK_ARG(k >= 1 && k <= df3d::KMAX, "k must be in [1, 16]");
    DF3D_CHECK_ARG(((h & (h - 1)) == 0) && ((w & (w - 1)) == 0), "h and w must be powers of two (reference heat-maps are 64 x 128)");
    DF3D_CHECK_ARG(h * w >= 64 && h * w <= 8192, "a plane must hold 64 .. 8192 cells (it is staged in LDS, 128 cells per lane)");
    if (n == 0) return DF3D_OK;
    DF3D_CHECK_ARG(hm_dev && count_dev && pts_dev && val_dev, "null pointer");
    DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(hm_dev) & 15) == 0, "heat-maps must be 16-byte aligned");
    const long long planes = (long long)n * joints;
    DF3D_CHECK_ARG(planes < (1ll << 31), "too many planes");
    const int wshift = __builtin_ctz((unsigned)w);
    hipLaunchKernelGGL(df3d::peaks_kernel<true>, dim3((unsigned)planes), dim3(df3d::PEAK_BLOCK), sizeof(float) * h * w,
                       df3d::as_stream(stream), hm_dev, h * w, w, wshift, k, 1.0f / (float)h, 1.0f / (float)w, count_dev, pts_dev, val_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
