// a11 constant-length leg fit (the model is this project's own specification, defined in float64 by
// tests/leg_fit_oracle.py): a chain of four fixed segment lengths fitted to a leg's measured joints by a damped Newton method on
// the product of four unit spheres.
//
// leg_fit_kernel: one lane per (frame, leg), 64 frames (384 lanes, six waves) per block, joint_angles_kernel's geometry.  The lane
// reads its leg's five joints (15 contiguous doubles), its four lengths and its anchor, iterates in registers and writes 15 doubles,
// one cost and its two info words as one 8-byte store.  A lane reads its leg before it writes it and touches no other leg, so the
// output may be the input.  One pass of the loop is one trial: residuals, tangent bases, gradient, the 8 x 8 system
// (H + lambda D) delta = -g formed column by column inside an unrolled Cholesky factorisation (36 entries), the solve, the
// retracted trial and its cost.  A rejected trial raises lambda and the next pass rebuilds the same system from the unchanged
// directions -- the same numbers the oracle keeps, so that H needs no second copy in registers.  Lanes leave the loop one by one; a
// wave runs until its slowest lane is done.  Every array is indexed by unrolled constants: no scratch, no LDS, no atomics.
//
// Six waves per block leave a lane 256 registers, and the factor (72), the solution (16), the directions (24) and the lengths (8) are
// alive through the factorisation whatever is done.  What else the pass needs is therefore not carried across it: the tangent
// bases are built a second time for the trial, and the targets are read again from the cache (see pin()).  All float64, default
// contraction.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int JOINTS = 38;
constexpr int LEGS = 6;
constexpr int FRAMES_PER_BLOCK = 64;
constexpr int THREADS = FRAMES_PER_BLOCK * LEGS;   // 384
constexpr double TINY = 1e-18;                     // relative bound on a squared start segment
constexpr double TOL = 1e-9;
constexpr double SLACK = 1e-12;                    // a trial is accepted when E' <= E (1 + SLACK): rounding must not reject a last step
constexpr double LAMBDA_MIN = 1e-3, LAMBDA_MAX = 1e12;
constexpr int NOT_FITTED = -1, CONVERGED = 0, OUT_OF_ITERATIONS = 1, STALLED = 2, RUNNING = -2;

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 axpy(double s, V3 a, V3 b) { return {s * a.x + b.x, s * a.y + b.y, s * a.z + b.z}; }
__device__ __forceinline__ V3 scale(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 load3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void store3(double* p, V3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
__device__ __forceinline__ bool finite3(V3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// all three coordinates exactly zero (the DLT's "fewer than two views"), or any of them not finite: section 14's rule
__device__ __forceinline__ bool missing(V3 p) { return (p.x == 0.0 && p.y == 0.0 && p.z == 0.0) || !finite3(p); }

// sum_k |c_k - t_k|^2 of the chain c_k = sum_{i <= k} len_i d_i
__device__ __forceinline__ double chain_cost(const V3 (&d)[4], const double (&len)[4], const V3 (&t)[4]) {
    V3 c = {0.0, 0.0, 0.0};
    double E = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c = axpy(len[k], d[k], c);
        const V3 r = sub(c, t[k]);
        E += dot(r, r);
    }
    return E;
}

// the tangent basis of the unit vector d, scaled by `len`: u1 = len (d x e)/|d x e| with e the axis of the smallest |component|
// (ties: the lowest index), u2 = d x u1
__device__ __forceinline__ void scaled_basis(V3 d, double len, V3& u1, V3& u2) {
    const double ax = fabs(d.x), ay = fabs(d.y), az = fabs(d.z);
    const bool ex = ax <= ay && ax <= az, ey = !ex && ay <= az;
    const V3 n = ex ? V3{0.0, d.z, -d.y} : ey ? V3{-d.z, 0.0, d.x} : V3{d.y, -d.x, 0.0};
    u1 = scale(len / sqrt(dot(n, n)), n);
    u2 = cross(d, u1);
}

// An empty volatile statement that claims to rewrite a value (no instruction is emitted).  It hides the value's origin from the
// optimiser: what is computed or loaded through it afterwards is computed or loaded again, rather than kept in registers from an
// earlier, identical computation or moved out of the loop
__device__ __forceinline__ void pin(size_t& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(V3& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z)); }

// index of entry (i, j), j <= i, of a symmetric 8 x 8 matrix kept as its lower triangle
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// the fixed lengths [6, 4] and the anchor [6, 3] travel as kernel arguments: the entry is asynchronous and its host arrays need
// not outlive the call
struct LegTables {
    double len[LEGS][4];
    double anchor[LEGS][3];
};

__global__ __launch_bounds__(THREADS) void leg_fit_kernel(const double* pts, long long T, const LegTables tab, int has_anchor, int max_iter,
                                                          double* out, double* __restrict__ cost, int* __restrict__ info) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;   // t * 6 + leg
    if (g >= T * LEGS) return;
    const long long t_ = g / LEGS;
    const int leg = (int)(g - t_ * LEGS);
    const int side = leg / 3;
    const size_t at = ((size_t)t_ * JOINTS + 19 * side + 5 * (leg - 3 * side)) * 3;
    V3 P[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) P[k] = load3(pts + at + 3 * k);
    double len[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) len[k] = tab.len[leg][k];
    const V3 p0 = has_anchor ? V3{tab.anchor[leg][0], tab.anchor[leg][1], tab.anchor[leg][2]} : P[0];

    bool fit = (has_anchor ? finite3(p0) : !missing(P[0])) && !missing(P[1]) && !missing(P[2]) && !missing(P[3]) && !missing(P[4]);
    V3 t[4], d[4];
    double tmax = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t[k] = sub(P[k + 1], p0);
        tmax = fmax(tmax, dot(t[k], t[k]));
    }
    // The origin and the four targets are read again wherever the loop needs them, from the lines this lane has just brought into
    // the cache, through an offset whose origin is hidden so that the loads are not moved out of the loop: 30 registers that
    // would sit idle through the factorisation.  Nothing writes the leg before the loop has ended
    size_t again = at;
    const auto targets = [&](V3 (&tt)[4]) {
        pin(again);
        const V3 o = has_anchor ? V3{tab.anchor[leg][0], tab.anchor[leg][1], tab.anchor[leg][2]} : load3(pts + again);
#pragma unroll
        for (int k = 0; k < 4; ++k) tt[k] = sub(load3(pts + again + 3 * (k + 1)), o);
        return o;
    };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const V3 s = k ? sub(t[k], t[k - 1]) : t[0];
        const double ss = dot(s, s);
        fit = fit && ss > TINY * tmax;
        d[k] = scale(1.0 / sqrt(ss), s);
    }

    double lam = 0.0;
    int iters = fit ? 0 : -1;
    int status = !fit ? NOT_FITTED : max_iter == 0 ? OUT_OF_ITERATIONS : RUNNING;
    while (status == RUNNING) {
        // residuals r_k, their tail sums S_i = sum_{k >= i} r_k, the cost
        V3 S[4];
        double E = 0.0;
        {
            targets(t);
            V3 c = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c = axpy(len[k], d[k], c);
                S[k] = sub(c, t[k]);
                E += dot(S[k], S[k]);
            }
#pragma unroll
            for (int k = 2; k >= 0; --k) S[k] = add(S[k], S[k + 1]);
        }
        // tangent bases, scaled by the segment's length: every entry of g and H is then one dot product of these, and the loop
        // carries no table of length products
        V3 u[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            scaled_basis(d[i], len[i], u[i][0], u[i][1]);
        }
        // x = -g and the diagonal's curvature and damping shift: the last use of S
        double A[36], x[8], shift[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = -dot(u[i][0], S[i]);
            x[2 * i + 1] = -dot(u[i][1], S[i]);
            shift[i] = lam * ((double)(4 - i) * (len[i] * len[i])) - len[i] * dot(d[i], S[i]);
        }
        // A = H + lambda D = L L^T, column by column: column j of A is formed (H(r, j) = (4 - r / 2) u_r . u_j, r >= j) when the
        // Cholesky factorisation reaches it, so that tangent vector j is dead after it and the matrix is never held beside its
        // factor.  A pivot that is not > 0 rejects the trial (the arithmetic goes on, on NaN); the diagonal keeps its reciprocal
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            double p = (double)(4 - j / 2) * dot(u[j / 2][j % 2], u[j / 2][j % 2]) + shift[j / 2];
#pragma unroll
            for (int k = 0; k < j; ++k) p -= A[tri(j, k)] * A[tri(j, k)];
            ok = ok && p > 0.0;
            const double inv = 1.0 / sqrt(p);
            A[tri(j, j)] = inv;
#pragma unroll
            for (int r = j + 1; r < 8; ++r) {
                double s = (double)(4 - r / 2) * dot(u[r / 2][r % 2], u[j / 2][j % 2]);
#pragma unroll
                for (int k = 0; k < j; ++k) s -= A[tri(r, k)] * A[tri(j, k)];
                A[tri(r, j)] = s * inv;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double s = x[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= A[tri(i, k)] * x[k];
            x[i] = s * A[tri(i, i)];
        }
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            double s = x[i];
#pragma unroll
            for (int k = i + 1; k < 8; ++k) s -= A[tri(k, i)] * x[k];
            x[i] = s * A[tri(i, i)];
        }
        // the trial: d' = (d + B delta)/|.|, B delta = (delta / len) u.  The bases are built a second time, bit for bit the same: kept
        // through the factorisation, their 24 doubles would not fit the 256 registers of a lane beside the 36 of the factor
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pin(d[i]);
            scaled_basis(d[i], len[i], u[i][0], u[i][1]);
        }
        bool small = true;
        V3 dn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            small = small && fabs(x[2 * i]) <= TOL && fabs(x[2 * i + 1]) <= TOL;
            const double rl = 1.0 / len[i];
            const V3 v = axpy(x[2 * i + 1] * rl, u[i][1], axpy(x[2 * i] * rl, u[i][0], d[i]));
            dn[i] = scale(1.0 / sqrt(dot(v, v)), v);
        }
        targets(t);
        if (ok && (small || chain_cost(dn, len, t) <= E * (1.0 + SLACK))) {
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = dn[i];
            ++iters;
            lam = lam > LAMBDA_MIN ? lam / 10.0 : 0.0;
            status = small ? CONVERGED : iters == max_iter ? OUT_OF_ITERATIONS : RUNNING;
        } else {
            lam = fmax(10.0 * lam, LAMBDA_MIN);
            if (lam > LAMBDA_MAX) status = STALLED;
        }
    }

    // a fitted leg: the anchor and the chain; a leg that is not fitted: the input's bits, read again (nothing has written them yet)
    // so that the loop above does not carry them in registers
    V3 c = {0.0, 0.0, 0.0};
    double E = 0.0;
    if (fit) {
        const V3 origin = targets(t);
        store3(out + at, origin);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c = axpy(len[k], d[k], c);
            const V3 r = sub(c, t[k]);
            E += dot(r, r);
            store3(out + at + 3 * (k + 1), add(origin, c));
        }
    } else if (out != pts) {
#pragma unroll
        for (int k = 0; k < 15; ++k) out[at + k] = pts[at + k];
    }
    cost[g] = fit ? E : __builtin_nan("");
    reinterpret_cast<int2*>(info)[g] = make_int2(status, iters);
}

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, long long na, const void* b, long long nb) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
}

constexpr long long MAX_T = 0x7fffffffLL * FRAMES_PER_BLOCK;   // one grid dimension

}  // namespace

extern "C" int df3d_leg_fit(const double* pts_dev, long long T, const double* lengths_host, const double* anchor_host, int max_iter,
                            double* out_pts_dev, double* cost_dev, int* info_dev, void* stream) {
    DF3D_CHECK_ARG(T >= 0 && T <= MAX_T, "T must be >= 0 (and at most 64 * (2^31 - 1))");
    DF3D_CHECK_ARG(max_iter >= 0, "max_iter must be >= 0");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(pts_dev && lengths_host && out_pts_dev && cost_dev && info_dev, "null pointer (only the anchor may be NULL)");
    LegTables tab;
    for (int leg = 0; leg < LEGS; ++leg) {
        for (int k = 0; k < 4; ++k) {
            const double v = lengths_host[leg * 4 + k];
            if (!(std::isfinite(v) && v > 0.0)) {
                df3d::set_error("%s: the length of leg %d, segment %d must be finite and > 0 (it is %g)", __func__, leg, k, v);
                return DF3D_EINVAL;
            }
            tab.len[leg][k] = v;
        }
        for (int k = 0; k < 3; ++k) {
            const double v = anchor_host ? anchor_host[leg * 3 + k] : 0.0;
            if (!std::isfinite(v)) {
                df3d::set_error("%s: the anchor of leg %d holds a non-finite coordinate", __func__, leg);
                return DF3D_EINVAL;
            }
            tab.anchor[leg][k] = v;
        }
    }
    DF3D_CHECK_ARG(((uintptr_t)info_dev & 7) == 0, "info must be 8-byte aligned (a leg's two words are one store)");
    const long long np = T * JOINTS * 3 * 8, nc = T * LEGS * 8, ni = T * LEGS * 2 * 4;   // bytes
    DF3D_CHECK_ARG(out_pts_dev == pts_dev || !overlap(out_pts_dev, np, pts_dev, np), "out must be pts itself (in place) or must not overlap pts");
    DF3D_CHECK_ARG(!overlap(cost_dev, nc, pts_dev, np) && !overlap(cost_dev, nc, out_pts_dev, np), "cost must not overlap pts or out");
    DF3D_CHECK_ARG(!overlap(info_dev, ni, pts_dev, np) && !overlap(info_dev, ni, out_pts_dev, np), "info must not overlap pts or out");
    DF3D_CHECK_ARG(!overlap(cost_dev, nc, info_dev, ni), "cost and info must not overlap each other");
    const long long blocks = (T + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
    hipLaunchKernelGGL(leg_fit_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, df3d::as_stream(stream), pts_dev, T, tab, anchor_host ? 1 : 0,
                       max_iter, out_pts_dev, cost_dev, info_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
