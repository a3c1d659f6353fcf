// a19 consensus triangulation over camera subsets (the model is this project's own specification, stated in
// float64 numpy by tests/consensus_oracle.py): per point (t, j) the DLT of every subset of the views with at least min_views cameras,
// each view's reprojection error against it, and the largest subset whose own views all lie within tau[j], ties to the smaller sum of
// squared errors, then to the smaller camera bitmask.  No atomics: two runs give the same bits.
//
// consensus_kernel: a block owns PB = 32 consecutive points.
//   1  the cameras go from the kernel argument into LDS (held as scalars, the 96 doubles spill); lane p < PB reads point p's
//      detections and its all-views point into LDS and forms the view mask; a point with fewer than two views is finished here
//      (status 0).  Then every (point, camera) pair builds that view's 4x4 contribution once (the ten upper
//      entries, DF3D_DLT_ADD_VIEW on a zeroed matrix) into LDS, where every subset that holds the view reads it.
//   2  lane 0 lays the work out: a point with n >= 2 views gets 2^n consecutive items, one per subset of its views, starting at a
//      multiple of 2^n.  Points of different n pack into the same passes: 32 points of 3 views are one pass of 256 lanes, one
//      point of 8 views is a pass of its own.
//   3  256 items per pass, one per lane: the subset's point (the sum of its views' contributions in ascending camera order,
//      DF3D_DLT_SOLVE's operations in dlt_solve(); the all-views item takes the caller's point), its views' errors and its key.  A point's items are an aligned
//      power-of-two run of lanes, so the total order reduces by an xor butterfly inside the wave and, for 128 and 256 items, through
//      four LDS slots across the waves.  The lane that holds the winning key (the all-views lane when no subset qualified) writes
//      the point's outputs.
// FUSED = false is df3d_consensus_candidates: the same passes and the same candidate(), every item's point and squared errors written
// and the point's outputs left out.
// count_slice_kernel / count_sum_kernel: status counted per joint over slices of 256 frames, the slices added in index order.
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "geometry_dev.h"

// Built with -ffp-contract=off (build.py): the projection, the error and the sum of squares are the oracle's operations one by one.

namespace {

using df3d::CamP;
using df3d::MAX_CAM;

constexpr int MAX_J = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / df3d::WAVE;
constexpr int PB = 32;        // points of a block
constexpr int SLICE = 256;    // frames of a count slice

struct Tau {
    double t[MAX_J];
};

struct Shared {
    double P[MAX_CAM][12];       // the cameras, copied from the kernel argument once: read from LDS (a broadcast), not held in scalar registers
    double row[PB][MAX_CAM], col[PB][MAX_CAM];
    double m[PB][MAX_CAM][10];   // upper triangle of a view's contribution, row-major
    double xf[PB][3];            // the all-views point
    int vm[PB];                  // view mask; 0 for a point outside the launch or with fewer than two views
    int start[PB + 1];
    double wsse[WAVES];
    unsigned wkey[WAVES];
};

struct Proj {
    double pu, pv;   // u / w, v / w
    double q, e;
};

// One camera's error against one point, the operations of tests/reproj_oracle.project and of the model one by one.
__device__ __forceinline__ Proj project_error(const double* P, double x0, double x1, double x2, double row, double col) {
    const double u = P[0] * x0 + P[1] * x1 + P[2] * x2 + P[3];
    const double v = P[4] * x0 + P[5] * x1 + P[6] * x2 + P[7];
    const double w = P[8] * x0 + P[9] * x1 + P[10] * x2 + P[11];
    Proj r;
    r.pu = u / w;
    r.pv = v / w;
    const double du = r.pu - col, dv = r.pv - row;
    r.q = du * du + dv * dv;
    r.e = sqrt(r.q);
    if (!(w > 0.0) || !isfinite(r.e)) r.e = __builtin_inf();
    return r;
}

// DF3D_DLT_SOLVE of csrc/geometry_dev.h operation by operation -- the scaling by 1 / trace, the cyclic sweeps of df3d::jacobi_rotate, the
// strict compare chain over the eigenvalues, the division by the last component -- with one difference in form: the eigenvector's column
// is picked by masks on the bits.  The macro's chain of conditional assignments is compiled into a dynamic index into v, which puts the
// 4 x 4 table into scratch (144 B per lane, as in triangulate_kernel); that is one solve per point there and the inner loop here.  The
// macro itself is left alone: df3d_triangulate must stay bit-identical.
__device__ __forceinline__ void dlt_solve(double (&a)[4][4], int nviews, double& out0, double& out1, double& out2) {
    if (nviews < 2) return;
    const double tr = a[0][0] + a[1][1] + a[2][2] + a[3][3];
    const double inv = tr > 0.0 ? 1.0 / tr : 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            a[i][j] *= inv;
            a[j][i] = a[i][j];
        }
    double v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        if (off < 1e-40) break;
        df3d::jacobi_rotate<0, 1>(a, v);
        df3d::jacobi_rotate<0, 2>(a, v);
        df3d::jacobi_rotate<0, 3>(a, v);
        df3d::jacobi_rotate<1, 2>(a, v);
        df3d::jacobi_rotate<1, 3>(a, v);
        df3d::jacobi_rotate<2, 3>(a, v);
    }
    double best = a[0][0];
    int col = 0;
    if (a[1][1] < best) best = a[1][1], col = 1;
    if (a[2][2] < best) best = a[2][2], col = 2;
    if (a[3][3] < best) best = a[3][3], col = 3;
    double e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long bits = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) bits |= __double_as_longlong(v[k][c]) & -(long long)(col == c);
        e[k] = __longlong_as_double(bits);
    }
    out0 = e[0] / e[3];
    out1 = e[1] / e[3];
    out2 = e[2] / e[3];
}

// a is better than b under the model's order.  A key is 0 for "does not qualify", else size << 8 | camera bitmask.
__device__ __forceinline__ bool better(double sa, unsigned ka, double sb, unsigned kb) {
    if (ka == 0) return false;
    if (kb == 0) return true;
    const unsigned na = ka >> 8, nb = kb >> 8;
    if (na != nb) return na > nb;
    if (sa != sb) return sa < sb;
    return ka < kb;
}

// The candidate `mask` (a subset of point p's views, `size` cameras, `full`: all of them): its point, the sum of its views' squared
// errors in ascending camera order and whether every one of them is finite and within tau.  q_out (may be null): q of camera c to
// q_out[c], +inf where the error is.
__device__ __forceinline__ void candidate(const Shared& L, int p, unsigned mask, int size, bool full, double tau, double& x0,
                                          double& x1, double& x2, double& sse, bool& qualifies, double* q_out) {
    x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (full) {
        x0 = L.xf[p][0], x1 = L.xf[p][1], x2 = L.xf[p][2];
    } else {
        double a[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][j] = 0.0;
#pragma unroll
        for (int c = 0; c < MAX_CAM; ++c)
            if (mask >> c & 1u) {
                int k = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = i; j < 4; ++j) a[i][j] += L.m[p][c][k++];
            }
        dlt_solve(a, size, x0, x1, x2);
    }
    sse = 0.0;
    qualifies = true;
#pragma unroll
    for (int c = 0; c < MAX_CAM; ++c)
        if (mask >> c & 1u) {
            const Proj r = project_error(L.P[c], x0, x1, x2, L.row[p][c], L.col[p][c]);
            sse += r.q;
            qualifies = qualifies && isfinite(r.e) && r.e <= tau;
            if (q_out) q_out[c] = isfinite(r.e) ? r.q : __builtin_inf();
        }
}

template <bool FUSED>
__global__ __launch_bounds__(THREADS) void consensus_kernel(CamP cams, Tau tau, const double* __restrict__ pts, const double* __restrict__ Xfull,
                                                            int ncam, long long TJ, int J, int min_views, double* __restrict__ X,
                                                            int* __restrict__ cameras, signed char* __restrict__ status, double* __restrict__ err,
                                                            double* __restrict__ fixed, double* __restrict__ cand_X, double* __restrict__ cand_q) {
    __shared__ Shared L;
    const int tid = threadIdx.x, lane = tid % df3d::WAVE, wave = tid / df3d::WAVE;
    const long long first = (long long)blockIdx.x * PB;

    if (tid < MAX_CAM * 12) L.P[tid / 12][tid % 12] = cams.p[tid / 12][tid % 12];
    // ---- 1: detections, view masks, points without a pair of views
    if (tid < PB) {
        const long long idx = first + tid;
        unsigned vm = 0;
        int n = 0;
#pragma unroll
        for (int c = 0; c < MAX_CAM; ++c) {
            double r = 0.0, cl = 0.0;
            if (idx < TJ && c < ncam) {
                r = pts[((size_t)c * TJ + idx) * 2];
                cl = pts[((size_t)c * TJ + idx) * 2 + 1];
                if (r != 0.0 && cl != 0.0) vm |= 1u << c, ++n;
            }
            L.row[tid][c] = r;
            L.col[tid][c] = cl;
        }
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        if (idx < TJ && n >= 2) f0 = Xfull[idx * 3], f1 = Xfull[idx * 3 + 1], f2 = Xfull[idx * 3 + 2];
        L.xf[tid][0] = f0, L.xf[tid][1] = f1, L.xf[tid][2] = f2;
        L.vm[tid] = n >= 2 ? (int)vm : 0;
        if (FUSED && idx < TJ && n < 2) {
            X[idx * 3] = 0.0, X[idx * 3 + 1] = 0.0, X[idx * 3 + 2] = 0.0;
            cameras[idx] = 0;
            status[idx] = 0;
#pragma unroll
            for (int c = 0; c < MAX_CAM; ++c)
                if (c < ncam) {
                    err[(size_t)c * TJ + idx] = 0.0;
                    if (fixed) {
                        fixed[((size_t)c * TJ + idx) * 2] = L.row[tid][c];
                        fixed[((size_t)c * TJ + idx) * 2 + 1] = L.col[tid][c];
                    }
                }
        }
    }
    __syncthreads();
    for (int k = tid; k < PB * MAX_CAM; k += THREADS) {
        const int p = k / MAX_CAM, c = k % MAX_CAM;
        if (L.vm[p] >> c & 1) {
            double a[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[i][j] = 0.0;
            int nv = 0;
            DF3D_DLT_ADD_VIEW(a, nv, L.P[c], L.row[p][c], L.col[p][c]);
            int e = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j) L.m[p][c][e++] = a[i][j];
        }
    }
    // ---- 2: the work layout
    if (tid == 0) {
        int s = 0;
        for (int p = 0; p < PB; ++p) {
            const int n = __popc((unsigned)L.vm[p]);
            const int cnt = n >= 2 ? 1 << n : 0;
            if (cnt) s = (s + cnt - 1) & ~(cnt - 1);
            L.start[p] = s;
            s += cnt;
        }
        L.start[PB] = s;
    }
    __syncthreads();
    const int total = L.start[PB];
    const int need = min_views > 2 ? min_views : 2;

    // ---- 3: the passes
    for (int base = 0; base < total; base += THREADS) {
        const int item = base + tid;
        int p = 0;
#pragma unroll
        for (int step = PB / 2; step > 0; step >>= 1)
            if (L.start[p + step] <= item) p += step;   // p + step <= PB - 1
        const unsigned vm = (unsigned)L.vm[p];
        const int n = __popc(vm);
        const int cnt = n >= 2 ? 1 << n : 0;
        const int lm = item - L.start[p];
        const bool on = item < total && lm >= 0 && lm < cnt;
        const int gs = on ? cnt : 1;
        unsigned mask = 0;
        if (on) {
            int b = 0;
#pragma unroll
            for (int c = 0; c < MAX_CAM; ++c)
                if (vm >> c & 1u) {
                    if (lm >> b & 1) mask |= 1u << c;
                    ++b;
                }
        }
        const int size = __popc(mask);
        const bool full = on && mask == vm;
        const long long idx = first + p;   // < TJ wherever `on`: a point outside the launch has no items
        const bool is_cand = on && size >= (FUSED ? need : 2);
        double x0 = 0.0, x1 = 0.0, x2 = 0.0, sse = 0.0;
        bool qualifies = false;
        if (is_cand) {
            double* q_out = FUSED ? nullptr : cand_q + ((size_t)idx << ncam) * ncam + (size_t)mask * ncam;
            candidate(L, p, mask, size, full, FUSED ? tau.t[idx % J] : 0.0, x0, x1, x2, sse, qualifies, q_out);
        } else if (full) {   // fewer views than min_views: the all-views lane still carries the point it may have to write
            x0 = L.xf[p][0], x1 = L.xf[p][1], x2 = L.xf[p][2];
        }
        if (!FUSED) {
            if (is_cand) {
                double* o = cand_X + (((size_t)idx << ncam) + mask) * 3;
                o[0] = x0, o[1] = x1, o[2] = x2;
            }
        }
        const unsigned mykey = qualifies ? ((unsigned)size << 8 | mask) : 0u;
        if (!qualifies) sse = 0.0;
        double bs = sse;
        unsigned bk = mykey;
#pragma unroll
        for (int o = 1; o < df3d::WAVE; o <<= 1) {
            const double os = __shfl_xor(bs, o);
            const unsigned ok = (unsigned)__shfl_xor((int)bk, o);
            if (o < gs && better(os, ok, bs, bk)) bs = os, bk = ok;
        }
        if (lane == 0) L.wsse[wave] = bs, L.wkey[wave] = bk;
        __syncthreads();
        if (gs > df3d::WAVE) {
            const int w0 = (tid & ~(gs - 1)) / df3d::WAVE, wn = gs / df3d::WAVE;   // w0 + wn <= WAVES: gs <= THREADS and the run is aligned
            for (int w = w0; w < w0 + wn; ++w)
                if (better(L.wsse[w], L.wkey[w], bs, bk)) bs = L.wsse[w], bk = L.wkey[w];
        }
        __syncthreads();
        // (the candidates entry runs the reduction too and writes nothing: one loop body, and its barriers keep the cameras in LDS)
        const bool writer = FUSED && on && (bk != 0 ? mykey == bk : full);
        if (writer) {
            const unsigned chosen = bk != 0 ? mask : vm;
            X[idx * 3] = x0, X[idx * 3 + 1] = x1, X[idx * 3 + 2] = x2;
            cameras[idx] = (int)chosen;
            status[idx] = bk == 0 ? 3 : (chosen == vm ? 1 : 2);
#pragma unroll
            for (int c = 0; c < MAX_CAM; ++c)
                if (c < ncam) {
                    const double r = L.row[p][c], cl = L.col[p][c];
                    double e = 0.0, fr = r, fc = cl;
                    if (vm >> c & 1u) {
                        const Proj pr = project_error(L.P[c], x0, x1, x2, r, cl);
                        e = pr.e;
                        if (!(chosen >> c & 1u)) fr = pr.pv, fc = pr.pu;
                    }
                    err[(size_t)c * TJ + idx] = e;
                    if (fixed) {
                        fixed[((size_t)c * TJ + idx) * 2] = fr;
                        fixed[((size_t)c * TJ + idx) * 2 + 1] = fc;
                    }
                }
        }
    }
}

// part[slice, j, s]: how often status s occurs at joint j in frames [slice SLICE, (slice + 1) SLICE)
__global__ __launch_bounds__(MAX_J) void count_slice_kernel(const signed char* __restrict__ status, int T, int J, long long* __restrict__ part) {
    const int j = threadIdx.x;
    if (j >= J) return;
    const long long t0 = (long long)blockIdx.x * SLICE, t1 = t0 + SLICE < T ? t0 + SLICE : T;
    long long n[4] = {0, 0, 0, 0};
    for (long long t = t0; t < t1; ++t) {
        const int s = status[t * J + j];
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] += s == k;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[((size_t)blockIdx.x * J + j) * 4 + k] = n[k];
}

__global__ __launch_bounds__(THREADS) void count_sum_kernel(const long long* __restrict__ part, int nslice, int J, long long* __restrict__ counts) {
    const int k = threadIdx.x;
    if (k >= J * 4) return;
    long long n = 0;
    for (int s = 0; s < nslice; ++s) n += part[(size_t)s * J * 4 + k];
    counts[k] = n;
}

// ------------------------------------------------------------------------------------------------------------------ host side
bool shape_ok(int ncam, int T, int J) { return ncam >= 1 && ncam <= MAX_CAM && J >= 1 && J <= MAX_J && T >= 0; }

long long slices_of(int T) { return ((long long)T + SLICE - 1) / SLICE; }

long long work_bytes_of(int T, int J) {
    const long long b = slices_of(T) * J * 4 * 8;
    return (b + 63) / 64 * 64;
}

}  // namespace

extern "C" long long df3d_consensus_work_bytes(int ncam, int T, int J) { return shape_ok(ncam, T, J) ? work_bytes_of(T, J) : 0; }

#define DF3D_CONSENSUS_SHAPE()                                                  \
    DF3D_CHECK_ARG(ncam >= 1 && ncam <= MAX_CAM, "ncam must be in [1, 8]");     \
    DF3D_CHECK_ARG(J >= 1 && J <= MAX_J, "J must be in [1, 64]");               \
    DF3D_CHECK_ARG(T >= 0, "T must be >= 0")

extern "C" int df3d_consensus_candidates(const double* P_host, const double* pts_px_dev, const double* X_full_dev, int ncam, int T, int J,
                                         double* cand_X_dev, double* cand_q_dev, void* stream) {
    DF3D_CONSENSUS_SHAPE();
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(P_host, "null pointer: P_host");
    const long long TJ = (long long)T * J, NM = 1LL << ncam;
    DF3D_BUFFERS({"pts_px", pts_px_dev, TJ * ncam * 16, 8}, {"X_full", X_full_dev, TJ * 24, 8}, {"cand_X", cand_X_dev, TJ * NM * 24, 8},
                 {"cand_q", cand_q_dev, TJ * NM * ncam * 8, 8});
    CamP cams;
    memset(&cams, 0, sizeof(cams));
    memcpy(cams.p, P_host, sizeof(double) * 12 * ncam);
    Tau tau;
    memset(&tau, 0, sizeof(tau));
    hipStream_t st = df3d::as_stream(stream);
    DF3D_HIP(hipMemsetAsync(cand_X_dev, 0, (size_t)(TJ * NM * 24), st));
    DF3D_HIP(hipMemsetAsync(cand_q_dev, 0, (size_t)(TJ * NM * ncam * 8), st));
    hipLaunchKernelGGL(consensus_kernel<false>, dim3((unsigned)((TJ + PB - 1) / PB)), dim3(THREADS), 0, st, cams, tau, pts_px_dev, X_full_dev, ncam, TJ,
                       J, 2, nullptr, nullptr, nullptr, nullptr, nullptr, cand_X_dev, cand_q_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_triangulate_consensus(const double* P_host, const double* pts_px_dev, const double* X_full_dev, int ncam, int T, int J,
                                          const double* tau_host, int min_views, double* X_dev, int* cameras_dev, signed char* status_dev,
                                          double* err_dev, double* fixed_px_dev, long long* counts_dev, void* work_dev, long long work_bytes,
                                          void* stream) {
    DF3D_CONSENSUS_SHAPE();
    DF3D_CHECK_ARG(min_views >= 2 && min_views <= MAX_CAM, "min_views must be in [2, 8]");
    Tau tau;
    memset(&tau, 0, sizeof(tau));
    for (int j = 0; tau_host && j < J; ++j) {
        DF3D_CHECK_ARG(tau_host[j] >= 0.0, "tau must be >= 0 and not NaN");
        tau.t[j] = tau_host[j];
    }
    if (T == 0) return DF3D_OK;
    DF3D_CHECK_ARG(P_host, "null pointer: P_host");
    DF3D_CHECK_ARG(tau_host, "null pointer: tau_host");
    DF3D_CHECK_ARG(work_bytes >= work_bytes_of(T, J), "work buffer too small (df3d_consensus_work_bytes)");
    const long long TJ = (long long)T * J;
    df3d::Range ranges[9] = {{"pts_px", pts_px_dev, TJ * ncam * 16, 8}, {"X_full", X_full_dev, TJ * 24, 8},       {"X", X_dev, TJ * 24, 8},
                             {"cameras", cameras_dev, TJ * 4, 4},       {"status", status_dev, TJ, 1},            {"err", err_dev, TJ * ncam * 8, 8},
                             {"work", work_dev, work_bytes_of(T, J), 8}};
    int count = 7;
    if (fixed_px_dev) ranges[count++] = {"fixed_px", fixed_px_dev, TJ * ncam * 16, 8};
    if (counts_dev) ranges[count++] = {"counts", counts_dev, (long long)J * 32, 8};
    if (const int rc = df3d::check_buffers(__func__, ranges, count)) return rc;
    CamP cams;
    memset(&cams, 0, sizeof(cams));
    memcpy(cams.p, P_host, sizeof(double) * 12 * ncam);
    hipStream_t st = df3d::as_stream(stream);
    hipLaunchKernelGGL(consensus_kernel<true>, dim3((unsigned)((TJ + PB - 1) / PB)), dim3(THREADS), 0, st, cams, tau, pts_px_dev, X_full_dev, ncam, TJ,
                       J, min_views, X_dev, cameras_dev, status_dev, err_dev, fixed_px_dev, nullptr, nullptr);
    if (counts_dev) {
        const int nslice = (int)slices_of(T);
        long long* part = static_cast<long long*>(work_dev);
        hipLaunchKernelGGL(count_slice_kernel, dim3((unsigned)nslice), dim3(MAX_J), 0, st, status_dev, T, J, part);
        hipLaunchKernelGGL(count_sum_kernel, dim3(1), dim3(THREADS), 0, st, part, nslice, J, counts_dev);
    }
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
