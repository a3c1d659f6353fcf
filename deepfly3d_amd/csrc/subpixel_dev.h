// Sub-pixel localisation of a heat-map peak from its 3 x 3 neighbourhood (the rule is this project's own
// specification, restated in float64 numpy by tests/subpixel_oracle.py and compared bit for bit).
//
// The operation order below IS the specification: include this header only from a file that build.py compiles with
// -ffp-contract=off (a fused multiply-add in det or in the Newton numerators rounds once where the rule rounds twice).
#pragma once
#include "common.h"

namespace df3d {

__device__ __forceinline__ double subpixel_axis(double g, double h) {
    if (!(h < 0.0)) return 0.0;
    const double d = -(g / h);
    return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
}

// The refined normalised (row, col) of cell (r, c) of an h x w plane; `at(rr, cc)` reads one value of the plane.  Cells on the border
// and cells with a non-finite value among the nine keep (r / h, c / w), the coordinates of the plain kernels, exactly.
template <class At>
__device__ __forceinline__ void subpixel_point(At at, int r, int c, int h, int w, double inv_h, double inv_w, float* row, float* col) {
    double dy = 0.0, dx = 0.0;
    if (r >= 1 && r + 1 < h && c >= 1 && c + 1 < w) {
        float q[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) q[a][b] = at(r + a - 1, c + b - 1);
        unsigned mag = 0;   // max of |x| as an integer, as in argmax_kernel: >= 0x7f800000 <=> an infinity or a NaN among the nine
        double n[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                mag = max(mag, __float_as_uint(q[a][b]) & 0x7fffffffu);
                n[a][b] = (double)q[a][b];
            }
        if (mag < 0x7f800000u) {
            const double gy = 0.5 * (n[2][1] - n[0][1]), gx = 0.5 * (n[1][2] - n[1][0]);
            const double hyy = (n[2][1] - 2.0 * n[1][1]) + n[0][1], hxx = (n[1][2] - 2.0 * n[1][1]) + n[1][0];
            const double hxy = 0.25 * (((n[2][2] - n[2][0]) - n[0][2]) + n[0][0]);
            const double det = hxx * hyy - hxy * hxy;
            bool newton = false;
            if (hxx < 0.0 && hyy < 0.0 && det > 0.0) {
                const double sx = -((hyy * gx - hxy * gy) / det), sy = -((hxx * gy - hxy * gx) / det);
                if (fabs(sx) <= 0.5 && fabs(sy) <= 0.5) {
                    newton = true;
                    dx = sx;
                    dy = sy;
                }
            }
            if (!newton) {   // each axis alone, clamped to the half cell
                dy = subpixel_axis(gy, hyy);
                dx = subpixel_axis(gx, hxx);
            }
        }
    }
    *row = (float)(((double)r + dy) * inv_h);
    *col = (float)(((double)c + dx) * inv_w);
}

}  // namespace df3d
