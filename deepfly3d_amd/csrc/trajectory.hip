// a20 trajectory triangulation (the model is this project's own specification, stated in float64 numpy by
// tests/trajectory_oracle.py): per joint, the 3-D points of a whole recording minimise the Huber loss of every view's reprojection error
// plus lambda times the squared second differences of the trajectory, by a damped Gauss-Newton iteration with IRLS weights.  float64,
// no atomics: two runs give the same bits.
//
// fit_kernel: one workgroup of 256 lanes per chain (joint), persistent over the whole iteration -- every synchronisation is a workgroup
// barrier and the host is never asked.  Its phases, each a loop of the lanes over the frames:
//   setup      views, anchors, the last / first anchor around every frame (a chunk per lane, the chunks joined through LDS), the active
//              frames, their status and start points
//   evaluate   one lane per frame: the views' projections against the cameras in LDS, their weights, H_t, g_t and the frame's cost
//              term (linearize_point: the oracle's operations one by one, this file is built with -ffp-contract=off), the smoothness
//              gradient and cost; the chain's cost is summed in the model's fixed order (chain_sum)
//   solve      (H + lambda K + mu I) d = -(g + lambda K X), 3 T scalar unknowns, half bandwidth 8 with its fill.  The chain is cut into
//              blocks of Bc frames whose last two frames are the block's separator.  eliminate_block: lane k eliminates the interior
//              of block k by the banded L D L^T in ascending order, carrying the "spike" (the coupling of the not yet eliminated rows
//              with the six unknowns of the separator to its left) and collecting that separator's Schur complement in registers.
//              reduce: the separators form a banded system of 6 nb unknowns, half bandwidth 11, eliminated pivot by pivot -- serial in
//              the pivots, the 77 updates of a pivot on 77 lanes -- and substituted back by one lane.  substitute_block: lane k substitutes
//              its interior back.  Frames past T (the last block's padding) and frames that are not active are identity rows.
//   trial      X + d, its cost, the decision (one per chain), the damping
// linearize_kernel / chain_sum_kernel / solve_kernel: the evaluate and solve phases alone, the same device functions, for the tests.
// solve_kernel's optional `ticks` receive the device's wall clock at the solve's phase boundaries (tests/perf/bench_trajectory.py).
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "geometry_dev.h"

namespace {

using df3d::CamP;
using df3d::MAX_CAM;

constexpr int MAX_J = 64;
constexpr int THREADS = 256;
constexpr int MAX_T = 1 << 20;
constexpr int BLOCK_MIN = 3, BLOCK_MAX = 1 << 20;
// the damped branch's constants (csrc/leg_fit.hip names them alike); their values are config.TRAJECTORY_*, which the oracle reads
constexpr double TOL = 1e-8;
constexpr double SLACK = 1e-12;
constexpr double MU_INIT = 1e-3, MU_MIN = 1e-6, MU_MAX = 1e12;
constexpr int MAX_ITER = 300;
constexpr int CONVERGED = 0, OUT_OF_ITERATIONS = 1, STALLED = 2, RUNNING = -2;

struct Lam {
    double v[MAX_J];
};

struct Shared {
    double P[MAX_CAM][12];   // the cameras, read from LDS (a broadcast): held as scalars they spill
    double red[THREADS];
    int ia[THREADS], ib[THREADS];
    long long cnt[5][THREADS / df3d::WAVE];
};

struct Lin {
    double H[6], g[3], cost;
};

// The views of point idx against (x0, x1, x2): tests/trajectory_oracle.linearize for one point.  weight / err (may be null): [ncam, TJ].
__device__ __forceinline__ void linearize_point(const double (*P)[12], const double* __restrict__ pts, int ncam, long long TJ, long long idx,
                                                double x0, double x1, double x2, double delta, Lin& o, double* __restrict__ weight,
                                                double* __restrict__ err, bool report) {
#pragma unroll
    for (int k = 0; k < 6; ++k) o.H[k] = 0.0;
    o.g[0] = o.g[1] = o.g[2] = 0.0;
    o.cost = 0.0;
    for (int c = 0; c < ncam; ++c) {
        const double row = pts[((size_t)c * TJ + idx) * 2], col = pts[((size_t)c * TJ + idx) * 2 + 1];
        const bool view = row != 0.0 && col != 0.0;
        const double* Pc = P[c];
        const double u = Pc[0] * x0 + Pc[1] * x1 + Pc[2] * x2 + Pc[3];
        const double v = Pc[4] * x0 + Pc[5] * x1 + Pc[6] * x2 + Pc[7];
        const double w = Pc[8] * x0 + Pc[9] * x1 + Pc[10] * x2 + Pc[11];
        const double pu = u / w, pv = v / w;
        const double du = pu - col, dv = pv - row;
        const double q = du * du + dv * dv;
        const double e = sqrt(q);
        const bool valid = view && w > 0.0 && isfinite(e);
        const bool inl = e <= delta;
        const double wt = inl ? 1.0 : delta / e;
        const double rho = inl ? q : 2.0 * delta * e - delta * delta;
        if (valid) {
            const double ju0 = (Pc[0] - pu * Pc[8]) / w, ju1 = (Pc[1] - pu * Pc[9]) / w, ju2 = (Pc[2] - pu * Pc[10]) / w;
            const double jv0 = (Pc[4] - pv * Pc[8]) / w, jv1 = (Pc[5] - pv * Pc[9]) / w, jv2 = (Pc[6] - pv * Pc[10]) / w;
            o.H[0] = o.H[0] + wt * (ju0 * ju0 + jv0 * jv0);
            o.H[1] = o.H[1] + wt * (ju0 * ju1 + jv0 * jv1);
            o.H[2] = o.H[2] + wt * (ju0 * ju2 + jv0 * jv2);
            o.H[3] = o.H[3] + wt * (ju1 * ju1 + jv1 * jv1);
            o.H[4] = o.H[4] + wt * (ju1 * ju2 + jv1 * jv2);
            o.H[5] = o.H[5] + wt * (ju2 * ju2 + jv2 * jv2);
            o.g[0] = o.g[0] + wt * (ju0 * du + jv0 * dv);
            o.g[1] = o.g[1] + wt * (ju1 * du + jv1 * dv);
            o.g[2] = o.g[2] + wt * (ju2 * du + jv2 * dv);
            o.cost = o.cost + rho;
        }
        if (report) {
            weight[(size_t)c * TJ + idx] = valid ? wt : 0.0;
            err[(size_t)c * TJ + idx] = view ? (valid ? e : __builtin_inf()) : 0.0;
        }
    }
}

// The model's chain sum of f[t J + j], t < T: every lane of the workgroup calls it; red is LDS of THREADS doubles.
__device__ __forceinline__ double chain_sum(const double* __restrict__ f, int T, int J, int j, double* red) {
    const int tid = threadIdx.x;
    double p = 0.0;
    for (int t = tid; t < T; t += THREADS) p = p + f[(size_t)t * J + j];
    red[tid] = p;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------------------- one chain's solve
struct Chain {
    int T, J, j, Bc, nb;
    double lam;
    const signed char* seg;   // [T, J]: non-zero where the frame is active
    double *band, *spike, *rhs, *SL, *rL, *Rb, *Rr;   // this chain's part of the work buffer: 27 Tp, 18 Tp, 3 Tp, 21 nb, 6 nb, 72 nb, 6 nb
};

__device__ __forceinline__ bool active(const Chain& c, int t) { return t >= 0 && t < c.T && c.seg[(size_t)t * c.J + c.j] != 0; }
__device__ __forceinline__ double centre(const Chain& c, int t) { return active(c, t - 1) && active(c, t) && active(c, t + 1) ? 1.0 : 0.0; }

__host__ __device__ inline int block_frames_of(int T, int block_frames) {
    const int floor3 = T > BLOCK_MIN ? T : BLOCK_MIN;
    return block_frames < floor3 ? block_frames : floor3;
}
__host__ __device__ inline int blocks_of(int T, int Bc) { return (T + Bc - 1) / Bc; }
__host__ __device__ inline long long chain_doubles(int T, int block_frames) {
    const long long Bc = block_frames_of(T, block_frames), nb = blocks_of(T, (int)Bc);
    return 48 * nb * Bc + 105 * nb;
}

__device__ __forceinline__ Chain chain_of(double* solve_work, int T, int J, int j, int block_frames, double lam, const signed char* seg) {
    Chain c;
    c.T = T, c.J = J, c.j = j, c.lam = lam, c.seg = seg;
    c.Bc = block_frames_of(T, block_frames);
    c.nb = blocks_of(T, c.Bc);
    const size_t Tp = (size_t)c.nb * c.Bc;
    double* w = solve_work + (size_t)j * (48 * Tp + 105 * (size_t)c.nb);
    c.band = w, w += 27 * Tp;
    c.spike = w, w += 18 * Tp;
    c.rhs = w, w += 3 * Tp;
    c.SL = w, w += 21 * (size_t)c.nb;
    c.rL = w, w += 6 * (size_t)c.nb;
    c.Rb = w, w += 72 * (size_t)c.nb;
    c.Rr = w;
    return c;
}

// A and b of the chain in band form: H [T, J, 6], G [T, J, 3] the whole gradient.  Every row of the padded chain is written.
__device__ __forceinline__ void assemble(const Chain& c, const double* __restrict__ H, const double* __restrict__ G, double mu) {
    const int Tp = c.nb * c.Bc;
    for (int t = threadIdx.x; t < Tp; t += THREADS) {
        const bool a = active(c, t);
        const double cb = centre(c, t - 1), cc = centre(c, t), ca = centre(c, t + 1);
        const double kd = cb + 4.0 * cc + ca, k1 = -2.0 * (cc + ca), k2 = ca;
        const size_t at = (size_t)t * c.J + c.j;
        double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        if (a) {
#pragma unroll
            for (int k = 0; k < 6; ++k) h[k] = H[at * 6 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = G[at * 3 + k];
        }
        const int first = t % c.Bc;   // the frame's place in its block
        const bool left = t >= c.Bc;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            double* row = c.band + ((size_t)t * 3 + x) * 9;
            const int d = x == 0 ? 0 : x == 1 ? 3 : 5;
            row[0] = a ? (h[d] + c.lam * kd) + mu : 1.0;
            row[1] = x < 2 ? h[d + 1] : 0.0;
            row[2] = x < 1 ? h[d + 2] : 0.0;
            row[3] = c.lam * k1;
            row[4] = 0.0, row[5] = 0.0;
            row[6] = c.lam * k2;
            row[7] = 0.0, row[8] = 0.0;
            double* sp = c.spike + ((size_t)t * 3 + x) * 6;
#pragma unroll
            for (int s = 0; s < 6; ++s) sp[s] = 0.0;
            if (left && first == 0) {
                sp[x] = c.lam * cb;                       // frame t - 2 with t: k2(t - 2) = c(t - 1)
                sp[3 + x] = c.lam * (-2.0 * (cb + cc));   // frame t - 1 with t: k1(t - 1)
            } else if (left && first == 1) {
                sp[3 + x] = c.lam * cb;                   // frame t - 2 with t, t - 2 being the separator's second frame
            }
            c.rhs[(size_t)t * 3 + x] = a ? -g[x] : 0.0;
        }
    }
}

__device__ __forceinline__ int tri6(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }   // a <= b < 6, 21 entries

// Lane-private: the interior rows of block k, in ascending order.  Returns false when a pivot was not > 0.
__device__ __forceinline__ bool eliminate_block(const Chain& c, int k) {
    const size_t r0 = (size_t)3 * k * c.Bc, r1 = r0 + (size_t)3 * (c.Bc - 2);
    const bool left = k > 0;
    double SL[21], rl[6];
#pragma unroll
    for (int e = 0; e < 21; ++e) SL[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) rl[e] = 0.0;
    bool ok = true;
    for (size_t i = r0; i < r1; ++i) {
        const int reach = 8 - (int)((i - r0) % 3);   // the last column of row i is the last row of the frame two ahead: inside the block
        double* row = c.band + i * 9;
        double u[9], us[6];
#pragma unroll
        for (int m = 0; m < 9; ++m) u[m] = row[m];
#pragma unroll
        for (int s = 0; s < 6; ++s) us[s] = left ? c.spike[i * 6 + s] : 0.0;
        const double p = u[0], z = c.rhs[i];
        ok = ok && p > 0.0;
#pragma unroll
        for (int m1 = 1; m1 < 9; ++m1)
            if (m1 <= reach) {
                const double l = u[m1] / p;
                double* r2 = c.band + (i + m1) * 9;
#pragma unroll
                for (int m2 = m1; m2 < 9; ++m2) r2[m2 - m1] -= l * u[m2];
                if (left) {
                    double* s2 = c.spike + (i + m1) * 6;
#pragma unroll
                    for (int s = 0; s < 6; ++s) s2[s] -= l * us[s];
                }
                c.rhs[i + m1] -= l * z;
            }
        if (left) {
#pragma unroll
            for (int s1 = 0; s1 < 6; ++s1) {
                const double l = us[s1] / p;
#pragma unroll
                for (int s2 = s1; s2 < 6; ++s2) SL[s1 * 6 - s1 * (s1 - 1) / 2 + (s2 - s1)] -= l * us[s2];
                rl[s1] -= l * z;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 21; ++e) c.SL[(size_t)k * 21 + e] = SL[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) c.rL[(size_t)k * 6 + e] = rl[e];
    return ok;
}

// Lane-private: x of the interior rows of block k in descending order, into rhs; the separators' rows of rhs hold their x already.
__device__ __forceinline__ void substitute_block(const Chain& c, int k) {
    const size_t r0 = (size_t)3 * k * c.Bc, r1 = r0 + (size_t)3 * (c.Bc - 2);
    const bool left = k > 0;
    double xl[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) xl[s] = left ? c.rhs[r0 - 6 + s] : 0.0;
    for (size_t i = r1; i-- > r0;) {
        const int reach = 8 - (int)((i - r0) % 3);
        const double* row = c.band + i * 9;
        double x = c.rhs[i];
#pragma unroll
        for (int m = 1; m < 9; ++m)
            if (m <= reach) x -= row[m] * c.rhs[i + m];
        if (left) {
#pragma unroll
            for (int s = 0; s < 6; ++s) x -= c.spike[i * 6 + s] * xl[s];
        }
        c.rhs[i] = x / row[0];
    }
}

// The whole solve of one chain by its workgroup: d = A^-1 b into c.rhs (3 Tp values).  Returns whether every pivot was > 0 (the same
// value on every lane).  Every lane of the workgroup calls it.
__device__ __forceinline__ bool chain_solve(const Chain& c, const double* __restrict__ H, const double* __restrict__ G, double mu,
                                            long long* __restrict__ ticks = nullptr) {
    const int tid = threadIdx.x;
    assemble(c, H, G, mu);
    __syncthreads();
    if (ticks && tid == 0) ticks[0] = wall_clock64();
    bool ok = true;
    for (int k = tid; k < c.nb; k += THREADS) ok = eliminate_block(c, k) && ok;
    __syncthreads();
    if (ticks && tid == 0) ticks[1] = wall_clock64();
    // the separators' system: row (k, s) = unknown 6 k + s, columns up to the end of separator k + 1
    const int n = 6 * c.nb;
    for (int e = tid; e < n; e += THREADS) {
        const int k = e / 6, s = e % 6;
        const size_t R = (size_t)3 * ((size_t)k * c.Bc + c.Bc - 2) + s;
        const bool next = k + 1 < c.nb;
        double* out = c.Rb + (size_t)e * 12;
        for (int m = 0; m < 12; ++m) {
            double v = 0.0;
            if (s + m < 6) {
                v = c.band[R * 9 + m];
                if (next) v += c.SL[(size_t)(k + 1) * 21 + tri6(s, s + m)];
            } else if (next && s + m < 12) {
                const int s2 = s + m - 6;                                   // in [0, 6)
                const size_t R2 = (size_t)3 * ((size_t)(k + 1) * c.Bc + c.Bc - 2) + s2;
                v = c.spike[R2 * 6 + s];
            }
            out[m] = v;
        }
        c.Rr[e] = c.rhs[R] + (next ? c.rL[(size_t)(k + 1) * 6 + s] : 0.0);
    }
    __syncthreads();
    // lane -> (m1, m2), 1 <= m1 <= m2 <= 11 (66 pairs), or the right-hand side of row m1 (11 more)
    int m1 = 0, m2 = 0;
    bool is_rhs = false;
    if (tid < 66) {
        int q = tid;
        m1 = 1;
        while (q >= 12 - m1) q -= 12 - m1, ++m1;
        m2 = m1 + q;
    } else if (tid < 77) {
        m1 = tid - 65, is_rhs = true;
    }
    for (int i = 0; i < n; ++i) {
        const double p = c.Rb[(size_t)i * 12];
        ok = ok && p > 0.0;
        if (m1 > 0 && i + m1 < n) {
            const double l = c.Rb[(size_t)i * 12 + m1] / p;
            if (is_rhs)
                c.Rr[i + m1] -= l * c.Rr[i];
            else
                c.Rb[(size_t)(i + m1) * 12 + (m2 - m1)] -= l * c.Rb[(size_t)i * 12 + m2];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int i = n - 1; i >= 0; --i) {
            double x = c.Rr[i];
            for (int m = 1; m < 12 && i + m < n; ++m) x -= c.Rb[(size_t)i * 12 + m] * c.Rr[i + m];
            c.Rr[i] = x / c.Rb[(size_t)i * 12];
        }
    }
    __syncthreads();
    for (int e = tid; e < n; e += THREADS) {
        const int k = e / 6, s = e % 6;
        c.rhs[(size_t)3 * ((size_t)k * c.Bc + c.Bc - 2) + s] = c.Rr[e];
    }
    __syncthreads();
    if (ticks && tid == 0) ticks[2] = wall_clock64();
    for (int k = tid; k < c.nb; k += THREADS) substitute_block(c, k);
    const bool all = __syncthreads_and(ok) != 0;
    if (ticks && tid == 0) ticks[3] = wall_clock64();
    return all;
}

// ------------------------------------------------------------------------------------------------------------------ the kernels
__global__ __launch_bounds__(THREADS) void linearize_kernel(CamP cams, const double* __restrict__ pts, const double* __restrict__ X, int ncam,
                                                            long long TJ, double delta, double* __restrict__ H, double* __restrict__ g,
                                                            double* __restrict__ weight, double* __restrict__ err, double* __restrict__ fcost) {
    __shared__ double P[MAX_CAM][12];
    const int tid = threadIdx.x;
    if (tid < MAX_CAM * 12) P[tid / 12][tid % 12] = cams.p[tid / 12][tid % 12];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * THREADS + tid;
    if (idx >= TJ) return;
    Lin o;
    linearize_point(P, pts, ncam, TJ, idx, X[idx * 3], X[idx * 3 + 1], X[idx * 3 + 2], delta, o, weight, err, true);
#pragma unroll
    for (int k = 0; k < 6; ++k) H[idx * 6 + k] = o.H[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[idx * 3 + k] = o.g[k];
    fcost[idx] = o.cost;
}

__global__ __launch_bounds__(THREADS) void chain_sum_kernel(const double* __restrict__ f, int T, int J, double* __restrict__ out) {
    __shared__ double red[THREADS];
    const double s = chain_sum(f, T, J, blockIdx.x, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(THREADS) void solve_kernel(const double* __restrict__ H, const double* __restrict__ G,
                                                        const signed char* __restrict__ seg, int T, int J, Lam lam, double mu, int block_frames,
                                                        double* __restrict__ d, int* __restrict__ ok_out, long long* __restrict__ ticks, double* __restrict__ solve_work) {
    const int j = blockIdx.x;
    const Chain c = chain_of(solve_work, T, J, j, block_frames, lam.v[j], seg);
    const bool ok = chain_solve(c, H, G, mu, ticks ? ticks + 4 * j : nullptr);
    for (int e = threadIdx.x; e < 3 * T; e += THREADS) d[((size_t)(e / 3) * J + j) * 3 + e % 3] = c.rhs[e];
    if (threadIdx.x == 0) ok_out[j] = ok ? 1 : 0;
}

// The chain's cost at Xs, and with `lin` H and the whole gradient too.  f, H, G: [T, J, .].  Every lane of the workgroup calls it.
__device__ __forceinline__ double evaluate(Shared& L, const Chain& c, const double* __restrict__ pts, int ncam, double delta,
                                           const double* __restrict__ Xs, bool lin, double* __restrict__ H, double* __restrict__ G,
                                           double* __restrict__ f) {
    const long long TJ = (long long)c.T * c.J;
    for (int t = threadIdx.x; t < c.T; t += THREADS) {
        const size_t at = (size_t)t * c.J + c.j;
        double cost = 0.0;
        if (active(c, t)) {
            Lin o;
            linearize_point(L.P, pts, ncam, TJ, (long long)at, Xs[at * 3], Xs[at * 3 + 1], Xs[at * 3 + 2], delta, o, nullptr, nullptr, false);
            // s(t') = (X[t' - 1] - 2 X[t']) + X[t' + 1] where c(t'), else 0: the frames t - 2 .. t + 2 are read only where a centre needs them
            const double cb = centre(c, t - 1), cc = centre(c, t), ca = centre(c, t + 1);
            double sm = 0.0;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const size_t J3 = (size_t)c.J * 3;
                const double* q = Xs + at * 3 + x;
                const double sb = cb != 0.0 ? (q[-2 * (ptrdiff_t)J3] - 2.0 * q[-(ptrdiff_t)J3]) + q[0] : 0.0;
                const double sc = cc != 0.0 ? (q[-(ptrdiff_t)J3] - 2.0 * q[0]) + q[J3] : 0.0;
                const double sa = ca != 0.0 ? (q[0] - 2.0 * q[J3]) + q[2 * J3] : 0.0;
                if (lin) G[at * 3 + x] = o.g[x] + c.lam * ((sb + -2.0 * sc) + sa);
                sm = x == 0 ? sc * sc : sm + sc * sc;
            }
            cost = o.cost + (cc != 0.0 ? c.lam * sm : 0.0);
            if (lin) {
#pragma unroll
                for (int k = 0; k < 6; ++k) H[at * 6 + k] = o.H[k];
            }
        }
        f[at] = cost;
    }
    __syncthreads();
    return chain_sum(f, c.T, c.J, c.j, L.red);
}

__global__ __launch_bounds__(THREADS) void fit_kernel(CamP cams, Lam lam, const double* __restrict__ pts, const double* __restrict__ X0, int ncam,
                                                      int T, int J, double delta, int max_gap, int block_frames, double* __restrict__ X,
                                                      signed char* __restrict__ status, double* __restrict__ weight, double* __restrict__ err,
                                                      int* __restrict__ iterations, double* __restrict__ cost_out, long long* __restrict__ counts,
                                                      double* __restrict__ work) {
    __shared__ Shared L;
    const int tid = threadIdx.x, j = blockIdx.x;
    const size_t TJ = (size_t)T * J;
    // the work buffer: X trial, H, G, f, then la / fa (int), anchor / run bytes, then the chains' solve parts
    double* Xn = work;
    double* H = Xn + TJ * 3;
    double* G = H + TJ * 6;
    double* f = G + TJ * 3;
    int* la = reinterpret_cast<int*>(f + TJ);
    int* fa = la + TJ;
    unsigned char* anc = reinterpret_cast<unsigned char*>(fa + TJ);
    unsigned char* run = anc + TJ;
    double* solve_work = f + TJ + ((TJ * 10 + 63) / 64) * 8;   // 10 T J bytes rounded up to 64
    const Chain c = chain_of(solve_work, T, J, j, block_frames, lam.v[j], status);

    if (tid < MAX_CAM * 12) L.P[tid / 12][tid % 12] = cams.p[tid / 12][tid % 12];
    // ---- setup.  bit 0 of anc: anchor, bit 1: at least one view
    const int chunk = (T + THREADS - 1) / THREADS;
    const int b0 = tid * chunk < T ? tid * chunk : T, e0 = b0 + chunk < T ? b0 + chunk : T;
    int last = -1, first = T;
    for (int t = b0; t < e0; ++t) {
        const size_t at = (size_t)t * J + j;
        int n = 0;
        for (int cam = 0; cam < ncam; ++cam) n += pts[((size_t)cam * TJ + at) * 2] != 0.0 && pts[((size_t)cam * TJ + at) * 2 + 1] != 0.0;
        const bool a = n >= 2 && isfinite(X0[at * 3]) && isfinite(X0[at * 3 + 1]) && isfinite(X0[at * 3 + 2]);
        anc[at] = (unsigned char)((a ? 1 : 0) | (n >= 1 ? 2 : 0));
        if (a) {
            last = t;
            if (first == T) first = t;
        }
    }
    L.ia[tid] = last, L.ib[tid] = first;
    __syncthreads();
    int cl = -1, cf = T;
    for (int q = 0; q < tid; ++q) cl = L.ia[q] > cl ? L.ia[q] : cl;
    for (int q = tid + 1; q < THREADS; ++q) cf = L.ib[q] < cf ? L.ib[q] : cf;
    for (int t = b0; t < e0; ++t) {
        const size_t at = (size_t)t * J + j;
        if (anc[at] & 1) cl = t;
        la[at] = cl;
    }
    for (int t = e0 - 1; t >= b0; --t) {
        const size_t at = (size_t)t * J + j;
        if (anc[at] & 1) cf = t;
        fa[at] = cf;
        run[at] = (anc[at] & 1) || (la[at] >= 0 && cf < T && (long long)cf - la[at] - 1 <= max_gap);
    }
    __syncthreads();
    for (int t = tid; t < T; t += THREADS) {
        const size_t at = (size_t)t * J + j;
        bool r[7];   // run of t - 3 .. t + 3
#pragma unroll
        for (int o = 0; o < 7; ++o) {
            const int tt = t + o - 3;
            r[o] = tt >= 0 && tt < T && run[(size_t)tt * J + j] != 0;
        }
        const bool act = r[3] && ((r[1] && r[2]) || (r[2] && r[4]) || (r[4] && r[5]));
        const bool a = anc[at] & 1;
        status[at] = (signed char)(!act ? 0 : a ? 1 : (anc[at] & 2) ? 2 : 3);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            double v = X0[at * 3 + x];
            if (act && !a) {
                const int ta = la[at], tb = fa[at];   // both exist: the frame is in a run and no anchor
                const double A = X0[((size_t)ta * J + j) * 3 + x], B = X0[((size_t)tb * J + j) * 3 + x];
                const double w = (double)(t - ta) / (double)(tb - ta);
                v = A + (B - A) * w;
            }
            X[at * 3 + x] = v;
            Xn[at * 3 + x] = v;
        }
    }
    __syncthreads();

    // ---- the iteration: Xc the accepted iterate, Xt the trial; both are [T, J, 3] and swap on acceptance
    double* Xc = X;
    double* Xt = Xn;
    double E = evaluate(L, c, pts, ncam, delta, Xc, true, H, G, f);
    const double E0 = E;
    double mu = MU_INIT;
    int state = RUNNING, iters = 0, trials = 0;
    bool any = false;
    for (int t = tid; t < T; t += THREADS) any = any || status[(size_t)t * J + j] != 0;
    if (!__syncthreads_or(any)) state = CONVERGED;
    bool fresh = true;   // H and G belong to Xc
    while (state == RUNNING) {
        if (!fresh) evaluate(L, c, pts, ncam, delta, Xc, true, H, G, f);
        fresh = true;
        const bool ok = chain_solve(c, H, G, mu);
        ++trials;
        bool big = false;
        for (int t = tid; t < T; t += THREADS) {
            const size_t at = (size_t)t * J + j;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const double d = c.rhs[(size_t)t * 3 + x];
                big = big || !(fabs(d) < TOL);
                Xt[at * 3 + x] = Xc[at * 3 + x] + d;
            }
        }
        const bool small = !__syncthreads_or(big);
        const double En = evaluate(L, c, pts, ncam, delta, Xt, false, H, G, f);
        if (ok && (small || En <= E * (1.0 + SLACK))) {
            double* s = Xc;
            Xc = Xt, Xt = s;
            E = En;
            ++iters;
            mu = fmax(mu / 10.0, MU_MIN);
            fresh = false;
            state = small ? CONVERGED : RUNNING;
        } else {
            mu = 10.0 * mu;
            if (mu > MU_MAX) state = STALLED;
        }
        if (state == RUNNING && trials == MAX_ITER) state = OUT_OF_ITERATIONS;
    }

    // ---- outputs
    long long n[5] = {0, 0, 0, 0, 0};
    for (int t = tid; t < T; t += THREADS) {
        const size_t at = (size_t)t * J + j;
        int s = status[at];   // (the solve's segment table until here; from here on a frame's own lane alone reads and writes it)
        // a frame that is not active keeps the input's bits (its step was 0.0, but -0.0 + 0.0 is not -0.0)
        const double* src = s != 0 ? Xc : X0;
        const double x0 = src[at * 3], x1 = src[at * 3 + 1], x2 = src[at * 3 + 2];
        if (s != 0) {
            Lin o;
            linearize_point(L.P, pts, ncam, (long long)TJ, (long long)at, x0, x1, x2, delta, o, weight, err, true);
            if (state != CONVERGED) s = 4;
        } else {
            for (int cam = 0; cam < ncam; ++cam) weight[(size_t)cam * TJ + at] = 0.0, err[(size_t)cam * TJ + at] = 0.0;
        }
        X[at * 3] = x0, X[at * 3 + 1] = x1, X[at * 3 + 2] = x2;
#pragma unroll
        for (int k = 0; k < 5; ++k) n[k] += s == k;
        if (s == 4) status[at] = 4;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        long long v = n[k];
        for (int o = df3d::WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (tid % df3d::WAVE == 0) L.cnt[k][tid / df3d::WAVE] = v;
    }
    __syncthreads();
    if (tid < 5) {
        long long v = 0;
        for (int w = 0; w < THREADS / df3d::WAVE; ++w) v += L.cnt[tid][w];
        counts[(size_t)j * 5 + tid] = v;
    }
    if (tid == 0) {
        iterations[j] = iters;
        cost_out[(size_t)j * 2] = E0;
        cost_out[(size_t)j * 2 + 1] = E;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
long long work_bytes_of(int T, int J, int block_frames) {
    const long long TJ = (long long)T * J;
    return (13 * TJ + (TJ * 10 + 63) / 64 * 8 + (long long)J * chain_doubles(T, block_frames)) * 8;
}

void load_cams(CamP& cams, const double* P_host, int ncam) {
    memset(&cams, 0, sizeof(cams));
    memcpy(cams.p, P_host, sizeof(double) * 12 * ncam);
}

}  // namespace

#define DF3D_TRAJECTORY_SHAPE()                                                                      \
    DF3D_CHECK_ARG(J >= 1 && J <= MAX_J, "J must be in [1, 64]");                                    \
    DF3D_CHECK_ARG(T >= 0 && T <= MAX_T, "T must be in [0, 1048576]")
#define DF3D_TRAJECTORY_CAMS() DF3D_CHECK_ARG(ncam >= 1 && ncam <= MAX_CAM, "ncam must be in [1, 8]")
#define DF3D_TRAJECTORY_BLOCK() \
    DF3D_CHECK_ARG(block_frames >= BLOCK_MIN && block_frames <= BLOCK_MAX, "block_frames must be in [3, 1048576]")

extern "C" long long df3d_trajectory_work_bytes(int ncam, int T, int J, int block_frames) {
    const bool ok = ncam >= 1 && ncam <= MAX_CAM && J >= 1 && J <= MAX_J && T >= 0 && T <= MAX_T && block_frames >= BLOCK_MIN && block_frames <= BLOCK_MAX;
    return ok && T > 0 ? work_bytes_of(T, J, block_frames) : 0;
}

extern "C" int df3d_trajectory_linearize(const double* P_host, const double* pts_px_dev, const double* X_dev, int ncam, int T, int J, double delta,
                                         double* H_dev, double* g_dev, double* weight_dev, double* err_dev, double* cost_dev, void* work_dev,
                                         long long work_bytes, void* stream) {
    DF3D_TRAJECTORY_CAMS();
    DF3D_TRAJECTORY_SHAPE();
    DF3D_CHECK_ARG(delta >= 0.0, "delta must be >= 0 and not NaN");
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(P_host, "null pointer: P_host");
    const long long TJ = (long long)T * J;
    DF3D_CHECK_ARG(work_bytes >= TJ * 8, "work buffer too small (8 T J bytes)");
    DF3D_BUFFERS({"pts_px", pts_px_dev, TJ * ncam * 16, 8}, {"X", X_dev, TJ * 24, 8}, {"H", H_dev, TJ * 48, 8}, {"g", g_dev, TJ * 24, 8},
                 {"weight", weight_dev, TJ * ncam * 8, 8}, {"err", err_dev, TJ * ncam * 8, 8}, {"cost", cost_dev, (long long)J * 8, 8},
                 {"work", work_dev, TJ * 8, 8});
    CamP cams;
    load_cams(cams, P_host, ncam);
    hipStream_t st = df3d::as_stream(stream);
    double* f = static_cast<double*>(work_dev);
    hipLaunchKernelGGL(linearize_kernel, dim3((unsigned)((TJ + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, cams, pts_px_dev, X_dev, ncam, TJ, delta,
                       H_dev, g_dev, weight_dev, err_dev, f);
    hipLaunchKernelGGL(chain_sum_kernel, dim3((unsigned)J), dim3(THREADS), 0, st, f, T, J, cost_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_trajectory_solve(const double* H_dev, const double* g_dev, const signed char* segment_dev, int T, int J, const double* lambda_host,
                                     double mu, int block_frames, double* d_dev, int* ok_dev, long long* ticks_dev, void* work_dev, long long work_bytes,
                                     void* stream) {
    DF3D_TRAJECTORY_SHAPE();
    DF3D_TRAJECTORY_BLOCK();
    DF3D_CHECK_ARG(mu >= 0.0 && mu <= MU_MAX * 10.0, "mu must be in [0, 1e13]");
    Lam lam;
    memset(&lam, 0, sizeof(lam));
    for (int j = 0; lambda_host && j < J; ++j) {
        DF3D_CHECK_ARG(lambda_host[j] >= 0.0 && std::isfinite(lambda_host[j]), "lambda must be >= 0 and finite");
        lam.v[j] = lambda_host[j];
    }
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(lambda_host, "null pointer: lambda_host");
    const long long TJ = (long long)T * J, need = (long long)J * chain_doubles(T, block_frames) * 8;
    DF3D_CHECK_ARG(work_bytes >= need, "work buffer too small (df3d_trajectory_work_bytes)");
    df3d::Range ranges[7] = {{"H", H_dev, TJ * 48, 8}, {"g", g_dev, TJ * 24, 8}, {"segment", segment_dev, TJ, 1}, {"d", d_dev, TJ * 24, 8},
                             {"ok", ok_dev, (long long)J * 4, 4}, {"work", work_dev, need, 8}};
    int count = 6;
    if (ticks_dev) ranges[count++] = {"ticks", ticks_dev, (long long)J * 32, 8};
    if (const int rc = df3d::check_buffers(__func__, ranges, count)) return rc;
    hipLaunchKernelGGL(solve_kernel, dim3((unsigned)J), dim3(THREADS), 0, df3d::as_stream(stream), H_dev, g_dev, segment_dev, T, J, lam, mu,
                       block_frames, d_dev, ok_dev, ticks_dev, static_cast<double*>(work_dev));
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_triangulate_trajectory(const double* P_host, const double* pts_px_dev, const double* X0_dev, int ncam, int T, int J,
                                           const double* lambda_host, double delta, int max_gap, int block_frames, double* X_dev,
                                           signed char* status_dev, double* weight_dev, double* err_dev, int* iterations_dev, double* cost_dev,
                                           long long* counts_dev, void* work_dev, long long work_bytes, void* stream) {
    DF3D_TRAJECTORY_CAMS();
    DF3D_TRAJECTORY_SHAPE();
    DF3D_TRAJECTORY_BLOCK();
    DF3D_CHECK_ARG(delta >= 0.0, "delta must be >= 0 and not NaN");
    DF3D_CHECK_ARG(max_gap >= 0 && max_gap <= 1000000, "max_gap must be in [0, 1000000]");
    Lam lam;
    memset(&lam, 0, sizeof(lam));
    for (int j = 0; lambda_host && j < J; ++j) {
        DF3D_CHECK_ARG(lambda_host[j] >= 0.0 && std::isfinite(lambda_host[j]), "lambda must be >= 0 and finite");
        lam.v[j] = lambda_host[j];
    }
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(P_host, "null pointer: P_host");
    DF3D_CHECK_ARG(lambda_host, "null pointer: lambda_host");
    const long long TJ = (long long)T * J, need = work_bytes_of(T, J, block_frames);
    DF3D_CHECK_ARG(work_bytes >= need, "work buffer too small (df3d_trajectory_work_bytes)");
    DF3D_BUFFERS({"pts_px", pts_px_dev, TJ * ncam * 16, 8}, {"X0", X0_dev, TJ * 24, 8}, {"X", X_dev, TJ * 24, 8}, {"status", status_dev, TJ, 1},
                 {"weight", weight_dev, TJ * ncam * 8, 8}, {"error", err_dev, TJ * ncam * 8, 8}, {"iterations", iterations_dev, (long long)J * 4, 4},
                 {"cost", cost_dev, (long long)J * 16, 8}, {"counts", counts_dev, (long long)J * 40, 8}, {"work", work_dev, need, 8});
    CamP cams;
    load_cams(cams, P_host, ncam);
    hipLaunchKernelGGL(fit_kernel, dim3((unsigned)J), dim3(THREADS), 0, df3d::as_stream(stream), cams, lam, pts_px_dev, X0_dev, ncam, T, J, delta,
                       max_gap, block_frames, X_dev, status_dev, weight_dev, err_dev, iterations_dev, cost_dev, counts_dev,
                       static_cast<double*>(work_dev));
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
