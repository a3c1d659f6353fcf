// Device code shared by geometry.hip (a4 re-layout, a6 DLT triangulation) and pictorial.hip (pictorial-structures
// correction): the 19 -> 38 re-layout rule and the float64 DLT of one point.  One copy of each, so that a proposal the
// correction builds from the arg-max detections is bit-identical to what df3d_triangulate returns for them.
#pragma once
#include "common.h"

namespace df3d {

constexpr int MAX_CAM = 8;

struct CamP {
    double p[MAX_CAM][12];
};

// The re-layout rule of reference df3d/core.py:187-203 for the camera at position `pos` of the ordering and output
// joint j (0..37): the network joint (0..18) it reads, or -1 when that camera does not see j; *left is set for the
// three left-side cameras, whose columns are un-flipped (col -> 1 - col) on ALL 38 joints.
__device__ __forceinline__ int relayout_source(int pos, int j, bool* left) {
    const bool right = pos >= 0 && pos < 3;   // ordering[0:3] -> joints 0..18
    const bool lft = pos >= 4 && pos < 7;     // ordering[4:7] -> joints 19..37
    int src = -1;
    if (right && j < 19) src = j;
    if (lft && j >= 19) src = j - 19;
    if (pos == 2 && j >= 15) src = -1;       // ordering[2] cannot see antenna / stripes
    if (pos == 4 && j >= 19 + 15) src = -1;  // ordering[4] neither
    *left = lft;
    return src;
}

template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double app = a[P][P], aqq = a[Q][Q];
    // tiny off-diagonal relative to the diagonal: nothing to do
    if (fabs(apq) <= 1e-300) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    a[P][P] = app - t * apq;
    a[Q][Q] = aqq + t * apq;
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = a[k][P], akq = a[k][Q];
            a[k][P] = c * akp - s * akq;
            a[P][k] = a[k][P];
            a[k][Q] = s * akp + c * akq;
            a[Q][k] = a[k][Q];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// The float64 DLT of one point: the 4x4 normal matrix M = A^T A of the system (rows x*P2 - P0, y*P2 - P1 of every camera
// that sees the point) accumulated in registers one view at a time (DF3D_DLT_ADD_VIEW on a zeroed a[4][4], nviews = 0), then
// diagonalised (DF3D_DLT_SOLVE).
// one camera's detection in pixels: P is that camera's 3x4 matrix (12 doubles, row-major); a detection with a zero coordinate is
// "not seen" (the reference's convention).  A macro, so that it expands in the caller's own scope: as a function taking the
// matrix by reference it changes how triangulate_kernel is compiled, and df3d_triangulate must stay bit-identical.
#define DF3D_DLT_ADD_VIEW(a, nviews, P, row_px, col_px)                                   \
    do {                                                                                  \
        const double row = (row_px), col = (col_px);                                      \
        if (row != 0.0 && col != 0.0) {                                                   \
            ++(nviews);                                                                   \
            double r0[4], r1[4];                                                          \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {                               \
                r0[k] = col * (P)[8 + k] - (P)[k];     /* x * P[2] - P[0],  x = col_px */ \
                r1[k] = row * (P)[8 + k] - (P)[4 + k]; /* y * P[2] - P[1],  y = row_px */ \
            }                                                                             \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                 \
                _Pragma("unroll") for (int j = i; j < 4; ++j)                             \
                    (a)[i][j] += r0[i] * r0[j] + r1[i] * r1[j];                           \
        }                                                                                 \
    } while (0)

// The point: M is pre-scaled by 1/trace so the cyclic Jacobi rotations work on O(1) numbers (scaling does not move
// eigenvectors); the eigenvector of the smallest eigenvalue = the last right-singular vector of A.  out0..2 (declared by the
// caller, = 0.0) are left at 0 when fewer than two cameras saw the point.  A macro for the reason given above.
#define DF3D_DLT_SOLVE(a, nviews, out0, out1, out2)                                                                  \
    do {                                                                                                             \
        if ((nviews) >= 2) {                                                                                         \
            const double tr = (a)[0][0] + (a)[1][1] + (a)[2][2] + (a)[3][3];                                         \
            const double inv = tr > 0.0 ? 1.0 / tr : 1.0;                                                            \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                            \
                _Pragma("unroll") for (int j = i; j < 4; ++j) {                                                      \
                    (a)[i][j] *= inv;                                                                                \
                    (a)[j][i] = (a)[i][j];                                                                           \
                }                                                                                                    \
            double v[4][4];                                                                                          \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                            \
                _Pragma("unroll") for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;                        \
            for (int sweep = 0; sweep < 16; ++sweep) {                                                               \
                const double off = fabs((a)[0][1]) + fabs((a)[0][2]) + fabs((a)[0][3]) + fabs((a)[1][2]) +           \
                                   fabs((a)[1][3]) + fabs((a)[2][3]);                                                \
                if (off < 1e-40) break;                                                                              \
                df3d::jacobi_rotate<0, 1>(a, v);                                                                     \
                df3d::jacobi_rotate<0, 2>(a, v);                                                                     \
                df3d::jacobi_rotate<0, 3>(a, v);                                                                     \
                df3d::jacobi_rotate<1, 2>(a, v);                                                                     \
                df3d::jacobi_rotate<1, 3>(a, v);                                                                     \
                df3d::jacobi_rotate<2, 3>(a, v);                                                                     \
            }                                                                                                        \
            /* eigenvector of the smallest eigenvalue (select with a compare chain: no dynamic indexing) */          \
            double best = (a)[0][0];                                                                                 \
            double e0 = v[0][0], e1 = v[1][0], e2 = v[2][0], e3 = v[3][0];                                           \
            if ((a)[1][1] < best) { best = (a)[1][1]; e0 = v[0][1]; e1 = v[1][1]; e2 = v[2][1]; e3 = v[3][1]; }      \
            if ((a)[2][2] < best) { best = (a)[2][2]; e0 = v[0][2]; e1 = v[1][2]; e2 = v[2][2]; e3 = v[3][2]; }      \
            if ((a)[3][3] < best) { best = (a)[3][3]; e0 = v[0][3]; e1 = v[1][3]; e2 = v[2][3]; e3 = v[3][3]; }      \
            (out0) = e0 / e3;                                                                                        \
            (out1) = e1 / e3;                                                                                        \
            (out2) = e2 / e3;                                                                                        \
        }                                                                                                            \
    } while (0)

}  // namespace df3d
