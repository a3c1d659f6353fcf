// a10 leg joint angles and segment lengths from the triangulated pose (the model is this project's own
// specification, restated in float64 by tests/joint_angles_oracle.py).
//
// joint_angles_kernel: one lane per (frame, leg), 64 frames (384 lanes, six waves) per block.  The lane reads its leg's five joints
// -- 15 contiguous doubles; the three legs of a side are 45 contiguous doubles, so a wave's loads fill the cache lines they touch
// but for the 12 doubles of antenna and stripes between the sides -- and the body frame (one broadcast address for the whole
// grid when nframes == 1), forms the four segment vectors in leg coordinates (side-1 legs mirrored in y) and writes eight angles and
// four lengths as 16-byte stores: 64 + 32 contiguous bytes per lane, contiguous over the wave.  ~720 B read and 576 B written per
// frame; no LDS, no atomics, no scratch.  All float64, default contraction: the tests hold it to 1e-10 rad, not to the bit.
//
// body_frame_kernel: one lane per pose, the frame rule of section 14 on the six body-coxa joints.
#include <cstdint>

#include "common.h"

namespace {

constexpr int JOINTS = 38;
constexpr int LEGS = 6;
constexpr int FRAMES_PER_BLOCK = 64;
constexpr int THREADS = FRAMES_PER_BLOCK * LEGS;   // 384
constexpr double TINY = 1e-18;                     // relative bound on a squared sine below which a direction is undefined

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 load3(const double* p) { return {p[0], p[1], p[2]}; }

// all three coordinates exactly zero (the DLT's "fewer than two views"), or any of them not finite
__device__ __forceinline__ bool missing(V3 p) {
    return (p.x == 0.0 && p.y == 0.0 && p.z == 0.0) || !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z));
}

// atan2(|u x v|, u . v) in [0, pi]
__device__ __forceinline__ double bend(V3 u, V3 v) {
    const V3 n = cross(u, v);
    return atan2(sqrt(dot(n, n)), dot(u, v));
}

// the right-handed rotation about w that carries u's projection perpendicular to w onto v's; NaN where either projection vanishes
__device__ __forceinline__ double tors(V3 u, V3 w, V3 v) {
    const V3 wu = cross(w, u), wv = cross(w, v);
    const double ww = dot(w, w);
    if (dot(wu, wu) <= TINY * ww * dot(u, u) || dot(wv, wv) <= TINY * ww * dot(v, v)) return __builtin_nan("");
    return atan2(sqrt(ww) * dot(w, cross(u, v)), dot(wu, wv));
}

__global__ __launch_bounds__(THREADS) void joint_angles_kernel(const double* __restrict__ pts, long long T, const double* __restrict__ frames,
                                                               int per_frame, double* __restrict__ angles, double* __restrict__ lengths) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;   // t * 6 + leg
    if (g >= T * LEGS) return;
    const long long t = g / LEGS;
    const int leg = (int)(g - t * LEGS);
    const int side = leg / 3;
    const double* p = pts + ((size_t)t * JOINTS + 19 * side + 5 * (leg - 3 * side)) * 3;
    V3 P[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) P[k] = load3(p + 3 * k);
    const double* F = frames + (per_frame ? (size_t)t * 9 : 0);
    const V3 ex = load3(F), ey = load3(F + 3), ez = load3(F + 6);
    const bool frame_ok = isfinite(ex.x) && isfinite(ex.y) && isfinite(ex.z) && isfinite(ey.x) && isfinite(ey.y) && isfinite(ey.z) &&
                          isfinite(ez.x) && isfinite(ez.y) && isfinite(ez.z);
    const double sigma = side ? -1.0 : 1.0;
    const double nan = __builtin_nan("");

    V3 q[4];        // a, b, c, d in leg coordinates
    double len[4];
    bool ok[4];     // both ends present and a non-zero length
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const V3 v = sub(P[k + 1], P[k]);
        const bool ends = !missing(P[k]) && !missing(P[k + 1]);
        const double vv = dot(v, v);
        len[k] = ends ? sqrt(vv) : nan;
        ok[k] = ends && vv > 0.0 && frame_ok;
        q[k] = {dot(v, ex), sigma * dot(v, ey), dot(v, ez)};
    }
    const V3 a = q[0], b = q[1], c = q[2], d = q[3];
    double out[8];
    const double axz = a.x * a.x + a.z * a.z;
    out[0] = ok[0] ? atan2(a.y, hypot(a.x, a.z)) : nan;
    out[1] = ok[0] && axz > TINY * dot(a, a) ? atan2(a.x, -a.z) : nan;
    out[2] = ok[0] && ok[1] ? tors(V3{0.0, 1.0, 0.0}, a, b) : nan;
    out[3] = ok[0] && ok[1] ? bend(a, b) : nan;
    out[4] = ok[0] && ok[1] && ok[2] ? tors(a, b, c) : nan;
    out[5] = ok[1] && ok[2] ? bend(b, c) : nan;
    out[6] = ok[1] && ok[2] && ok[3] ? tors(b, c, d) : nan;
    out[7] = ok[2] && ok[3] ? bend(c, d) : nan;

    double2* A = reinterpret_cast<double2*>(angles + (size_t)g * 8);   // 64-byte aligned rows
#pragma unroll
    for (int k = 0; k < 4; ++k) A[k] = make_double2(out[2 * k], out[2 * k + 1]);
    if (lengths) {
        double2* L = reinterpret_cast<double2*>(lengths + (size_t)g * 4);
        L[0] = make_double2(len[0], len[1]);
        L[1] = make_double2(len[2], len[3]);
    }
}

__global__ __launch_bounds__(256) void body_frame_kernel(const double* __restrict__ pts, long long n, double* __restrict__ frames) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* p = pts + (size_t)i * JOINTS * 3;
    V3 C[2][3];
    bool ok = true;
    double cmax = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            C[s][l] = load3(p + (19 * s + 5 * l) * 3);
            ok = ok && !missing(C[s][l]);
            cmax = fmax(cmax, dot(C[s][l], C[s][l]));
        }
    }
    const double third = 1.0 / 3.0;
    const V3 m0 = {(C[0][0].x + C[0][1].x + C[0][2].x) * third, (C[0][0].y + C[0][1].y + C[0][2].y) * third, (C[0][0].z + C[0][1].z + C[0][2].z) * third};
    const V3 m1 = {(C[1][0].x + C[1][1].x + C[1][2].x) * third, (C[1][0].y + C[1][1].y + C[1][2].y) * third, (C[1][0].z + C[1][1].z + C[1][2].z) * third};
    const V3 dy = sub(m0, m1);   // side 1 to side 0
    const double dy2 = dot(dy, dy);
    ok = ok && dy2 > TINY * cmax;
    const double ry = 1.0 / sqrt(dy2);
    const V3 ey = {dy.x * ry, dy.y * ry, dy.z * ry};
    const V3 f = {0.5 * ((C[0][0].x + C[1][0].x) - (C[0][2].x + C[1][2].x)), 0.5 * ((C[0][0].y + C[1][0].y) - (C[0][2].y + C[1][2].y)),
                  0.5 * ((C[0][0].z + C[1][0].z) - (C[0][2].z + C[1][2].z))};   // hind to front
    const double fy = dot(f, ey);
    const V3 fp = {f.x - fy * ey.x, f.y - fy * ey.y, f.z - fy * ey.z};
    const double fp2 = dot(fp, fp);
    ok = ok && fp2 > TINY * cmax;
    const double rx = 1.0 / sqrt(fp2);
    const V3 ex = {fp.x * rx, fp.y * rx, fp.z * rx};
    const V3 ez = cross(ex, ey);
    const double nan = __builtin_nan("");
    double* F = frames + (size_t)i * 9;
    F[0] = ok ? ex.x : nan;
    F[1] = ok ? ex.y : nan;
    F[2] = ok ? ex.z : nan;
    F[3] = ok ? ey.x : nan;
    F[4] = ok ? ey.y : nan;
    F[5] = ok ? ey.z : nan;
    F[6] = ok ? ez.x : nan;
    F[7] = ok ? ez.y : nan;
    F[8] = ok ? ez.z : nan;
}

// whether [a, a + na) and [b, b + nb) doubles share a byte
bool overlap(const double* a, long long na, const double* b, long long nb) { return a < b + nb && b < a + na; }

constexpr long long MAX_T = 0x7fffffffLL * FRAMES_PER_BLOCK;   // one grid dimension

}  // namespace

extern "C" int df3d_body_frame(const double* pts_dev, long long n, double* frame_dev, void* stream) {
    DF3D_CHECK_ARG(n >= 0 && n <= MAX_T, "n must be >= 0 (and at most 64 * (2^31 - 1))");
    if (n == 0) return DF3D_OK;
    DF3D_CHECK_ARG(pts_dev && frame_dev, "null pointer");
    DF3D_CHECK_ARG(!overlap(frame_dev, n * 9, pts_dev, n * JOINTS * 3), "frame must not overlap pts");
    hipLaunchKernelGGL(body_frame_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, df3d::as_stream(stream), pts_dev, n, frame_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_joint_angles(const double* pts_dev, long long T, const double* frame_dev, long long nframes, double* angles_dev,
                                 double* lengths_dev, void* stream) {
    DF3D_CHECK_ARG(T >= 0 && T <= MAX_T, "T must be >= 0 (and at most 64 * (2^31 - 1))");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(pts_dev && frame_dev && angles_dev, "null pointer (only lengths may be NULL)");
    DF3D_CHECK_ARG(nframes == 1 || nframes == T, "nframes must be 1 (one frame for the recording) or T (one per pose)");
    DF3D_CHECK_ARG(((uintptr_t)angles_dev & 15) == 0 && ((uintptr_t)lengths_dev & 15) == 0, "angles and lengths must be 16-byte aligned");
    const long long np = T * JOINTS * 3, na = T * LEGS * 8, nl = lengths_dev ? T * LEGS * 4 : 0;
    DF3D_CHECK_ARG(!overlap(angles_dev, na, pts_dev, np) && !(nl && overlap(lengths_dev, nl, pts_dev, np)), "outputs must not overlap pts");
    DF3D_CHECK_ARG(!overlap(angles_dev, na, frame_dev, nframes * 9) && !(nl && overlap(lengths_dev, nl, frame_dev, nframes * 9)),
                   "outputs must not overlap the frames");
    DF3D_CHECK_ARG(!(nl && overlap(angles_dev, na, lengths_dev, nl)), "angles and lengths must not overlap each other");
    const long long blocks = (T + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
    hipLaunchKernelGGL(joint_angles_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, df3d::as_stream(stream), pts_dev, T, frame_dev,
                       nframes != 1 ? 1 : 0, angles_dev, lengths_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
