// a13 t-SNE behaviour map of the angle spectrograms (the model is this project's own specification, defined in
// float64 by tests/behaviour_map_oracle.py).  Every stage is its own entry, all float64, no atomics, every sum in a fixed order.
//
// bmap_prepare_kernel: one block per row of S.  p = (S / sum + floor) / (1 + D floor), L = log p, e = sum p L, and the row's
//     validity (every entry finite and >= 0, a finite sum > 0); an invalid row gets NaN.
// bmap_divergence_kernel: K[i, j] = max(0, e_i - sum_d PA[i, d] LB[j, d]) on the vector pipe.  A block of 256 threads owns a
//     128 x 64 tile of K and walks D in chunks of 16 through LDS (both operands stored d-major there); a thread carries an 8 x 4
//     micro-tile, so one chunk step reads 12 doubles from LDS for 32 multiply-adds.  Any M, N, D >= 1: the tile edges are
//     filled with zeros and masked on the way out.
// bmap_calibrate_kernel: one block per row.  The row of K stays in LDS (up to 16 384 doubles = 128 KiB) through the root search
//     for beta: a Newton step on H(beta) = log u, kept inside a bracket, every fourth step a bisection of the bracket.
// bmap_joint_kernel: P = (c + c^T) / (2N) with a zero diagonal, 32 x 32 tiles transposed through LDS.
// tsne_gradient_kernel: a block owns 4 rows i; lane t of the block owns the columns j = t, t + 256, ...: y_j sits in its
//     registers, the four y_i come from LDS as broadcasts, and P[i, j] is read once, coalesced along j, four columns (16 loads)
//     requested per lane before the first is used: the loop is bound by the bytes of P in flight.  Per row it leaves
//     sum P w (y_i - y_j), sum w^2 (y_i - y_j) and sum_{j != i} w in the workspace.
// tsne_update_kernel: every block sums the N row values of Z in the same fixed order, forms g and applies the gain, velocity
//     and position update to its 256 rows.
// bmap_cost_*: the row sums of P (log P - log w), of P and of w, then one block folds them into KL.
// bmap_place_kernel: y_t = sum_j c[t, j] Y[j], one block per row.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / df3d::WAVE;
constexpr int MAX_POINTS = 16384;   // calibration keeps a row of this many doubles in LDS; the dense N x N tables are 2 GB each here
constexpr int MAX_ROOT_STEPS = 400;

// Sum of v[k] over the block, in a fixed order, left in every thread.  red: WAVES * NV doubles of LDS.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int o = df3d::WAVE / 2; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o);
    __syncthreads();   // the previous call's readers are done with red
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = red[k];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += red[w * NV + k];
        v[k] = s;
    }
}

__device__ __forceinline__ double block_min(double v, double* red) {
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
#pragma unroll
    for (int o = df3d::WAVE / 2; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o));
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = fmin(s, red[w]);
    return s;
}

// ------------------------------------------------------------------------------------------------------------------ preparation
// NORMALISE: S -> p by the model's rule.  Otherwise the input is p itself and only L and e are written.
template <bool NORMALISE>
__global__ __launch_bounds__(THREADS) void bmap_prepare_kernel(const double* __restrict__ S, int D, double floor_, double* __restrict__ p,
                                                               double* __restrict__ logp, double* __restrict__ e, int* __restrict__ valid) {
    __shared__ double red[WAVES * 2];
    const long long t = blockIdx.x;
    const double* row = S + t * D;
    double scale = 1.0, add = 0.0;
    bool ok = true;
    if (NORMALISE) {
        double v[2] = {0.0, 0.0};
        for (int d = threadIdx.x; d < D; d += THREADS) {
            const double s = row[d];
            v[0] += s;
            if (!(isfinite(s) && s >= 0.0)) v[1] += 1.0;
        }
        block_sum(v, red);
        ok = v[1] == 0.0 && isfinite(v[0]) && v[0] > 0.0;
        scale = 1.0 / (1.0 + (double)D * floor_);
        add = floor_;
        if (ok) {
            double w[1] = {0.0};
            for (int d = threadIdx.x; d < D; d += THREADS) {
                const double q = (row[d] / v[0] + add) * scale;
                const double l = log(q);
                p[t * D + d] = q;
                logp[t * D + d] = l;
                w[0] += q * l;
            }
            block_sum(w, red);
            if (threadIdx.x == 0) {
                e[t] = w[0];
                valid[t] = 1;
            }
        } else {
            const double nan = __builtin_nan("");
            for (int d = threadIdx.x; d < D; d += THREADS) p[t * D + d] = logp[t * D + d] = nan;
            if (threadIdx.x == 0) {
                e[t] = nan;
                valid[t] = 0;
            }
        }
    } else {
        double w[1] = {0.0};
        for (int d = threadIdx.x; d < D; d += THREADS) {
            const double q = row[d];
            const double l = log(q);
            logp[t * D + d] = l;
            w[0] += q * l;
        }
        block_sum(w, red);
        if (threadIdx.x == 0) e[t] = w[0];
    }
}

// ------------------------------------------------------------------------------------------------------------------ divergence
constexpr int TM = 128, TN = 64, TD = 16, PADM = 4, PADN = 4;

__global__ __launch_bounds__(THREADS) void bmap_divergence_kernel(const double* __restrict__ pa, const double* __restrict__ ea, long long M,
                                                                  const double* __restrict__ lb, long long N, int D, double* __restrict__ K) {
    __shared__ double As[TD][TM + PADM];
    __shared__ double Bs[TD][TN + PADN];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long i0 = (long long)blockIdx.y * TM, j0 = (long long)blockIdx.x * TN;
    double acc[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int d0 = 0; d0 < D; d0 += TD) {
        // the chunk: A 128 x 16 (8 per thread), B 64 x 16 (4 per thread); a thread reads along d, the contiguous axis
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int el = q * THREADS + threadIdx.x, row = el >> 4, d = el & 15;
            const bool in = i0 + row < M && d0 + d < D;
            As[d][row] = in ? pa[(i0 + row) * D + d0 + d] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int el = q * THREADS + threadIdx.x, row = el >> 4, d = el & 15;
            const bool in = j0 + row < N && d0 + d < D;
            Bs[d][row] = in ? lb[(j0 + row) * D + d0 + d] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < TD; ++d) {
            double a[8], b[4];
#pragma unroll
            for (int r = 0; r < 8; ++r) a[r] = As[d][ty * 8 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = Bs[d][tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const long long i = i0 + ty * 8 + r;
        if (i >= M) break;
        const double ei = ea[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long j = j0 + tx * 4 + c;
            if (j < N) {
                const double k = ei - acc[r][c];
                K[i * N + j] = k < 0.0 ? 0.0 : k;   // a NaN stays a NaN
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ calibration
__global__ __launch_bounds__(THREADS) void bmap_calibrate_kernel(const double* __restrict__ K, int N, double target, double tol, double beta_max,
                                                                 const int* __restrict__ exclude, double* __restrict__ cond,
                                                                 double* __restrict__ beta_out, int* __restrict__ info_out) {
    extern __shared__ double krow[];   // K[i, :] - m
    __shared__ double red[WAVES * 3];
    const long long i = blockIdx.x;
    const int x = exclude ? exclude[i] : -1;
    const double* src = K + i * N;
    double m = INFINITY;
    for (int j = threadIdx.x; j < N; j += THREADS) {
        const double k = src[j];
        krow[j] = k;
        if (j != x) m = fmin(m, k);
    }
    m = block_min(m, red);
    double mean[1] = {0.0};
    for (int j = threadIdx.x; j < N; j += THREADS) {
        const double k = krow[j] - m;
        krow[j] = k;
        if (j != x) mean[0] += k;
    }
    block_sum(mean, red);
    const int n = N - (x >= 0 && x < N ? 1 : 0);
    int info = 0;
    double beta = beta_max, S = 0.0;
    // every thread runs the same scalar search on the block's sums
    if (!(mean[0] > 0.0)) {
        info = 1;   // every admitted entry ties at the minimum: H = log n at any beta
    } else {
        beta = fmin((double)n / mean[0], beta_max);
        double lo = 0.0, hi = -1.0;
        info = 2;   // cleared when the stopping rule is met
        for (int it = 0; it < MAX_ROOT_STEPS; ++it) {
            double v[3] = {0.0, 0.0, 0.0};
            for (int j = threadIdx.x; j < N; j += THREADS) {
                if (j == x) continue;
                const double k = krow[j];
                const double w = exp(-beta * k);
                v[0] += w;
                v[1] += k * w;
                v[2] += k * k * w;
            }
            block_sum(v, red);
            S = v[0];
            const double q = v[1] / S;
            const double diff = log(S) + beta * q - target;
            if (fabs(diff) <= tol) {
                info = 0;
                break;
            }
            if (diff > 0.0) {
                if (beta >= beta_max) {
                    info = 1;   // at least u entries tie at the minimum: no beta in (0, beta_max] reaches the target
                    break;
                }
                lo = beta;
            } else {
                hi = beta;
            }
            const double slope = -beta * (v[2] / S - q * q);
            double next = beta - diff / slope;
            if (hi < 0.0) {
                if (!(next > beta) || !(next <= 16.0 * beta)) next = next > beta ? 16.0 * beta : 2.0 * beta;
                next = fmin(next, beta_max);
            } else if ((it & 3) == 3 || !(next > lo && next < hi)) {
                next = lo > 0.0 && hi > 4.0 * lo ? sqrt(lo * hi) : 0.5 * (lo + hi);
            }
            beta = next;
        }
    }
    if (info & 1) {   // the reported condition: beta_max, the weights evaluated there
        beta = beta_max;
        double v[1] = {0.0};
        for (int j = threadIdx.x; j < N; j += THREADS)
            if (j != x) v[0] += exp(-beta * krow[j]);
        block_sum(v, red);
        S = v[0];
    }
    double* dst = cond + i * N;
    for (int j = threadIdx.x; j < N; j += THREADS) dst[j] = j == x ? 0.0 : exp(-beta * krow[j]) / S;
    if (threadIdx.x == 0) {
        beta_out[i] = beta;
        info_out[i] = info;
    }
}

// ------------------------------------------------------------------------------------------------------------------ joint table
__global__ __launch_bounds__(THREADS) void bmap_joint_kernel(const double* __restrict__ c, int N, double* __restrict__ P) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    for (int k = ty; k < 32; k += 8) {   // tile[a][b] = c[j0 + a, i0 + b]
        const int r = j0 + k, col = i0 + tx;
        tile[k][tx] = r < N && col < N ? c[(long long)r * N + col] : 0.0;
    }
    __syncthreads();
    const double twice = 2.0 * (double)N;
    for (int k = ty; k < 32; k += 8) {
        const int i = i0 + k, j = j0 + tx;
        if (i < N && j < N) P[(long long)i * N + j] = i == j ? 0.0 : (c[(long long)i * N + j] + tile[tx][k]) / twice;
    }
}

// ------------------------------------------------------------------------------------------------------------------ optimisation
constexpr int ROWS = 4;      // rows of P per block of the gradient kernel
constexpr int EXAGGERATION_ITERS = 250;   // config.BEHAVIOUR_EXAGGERATION_ITERATIONS
constexpr int DEPTH = 4;     // columns per lane whose P values are in flight together
constexpr int ACC = 5;       // per row: sum P w dx, sum P w dy, sum w^2 dx, sum w^2 dy, sum_{j != i} w

__global__ __launch_bounds__(THREADS) void tsne_gradient_kernel(const double* __restrict__ P, int N, const double2* __restrict__ Y,
                                                                double* __restrict__ work) {
    __shared__ double2 yi_s[ROWS];
    __shared__ double red[WAVES * ROWS * ACC];
    const int i0 = blockIdx.x * ROWS;
    if (threadIdx.x < ROWS) yi_s[threadIdx.x] = Y[i0 + (int)threadIdx.x < N ? i0 + (int)threadIdx.x : N - 1];
    __syncthreads();
    double acc[ROWS * ACC];
#pragma unroll
    for (int k = 0; k < ROWS * ACC; ++k) acc[k] = 0.0;
    const int rows = N - i0 < ROWS ? N - i0 : ROWS;
    // DEPTH columns per lane are requested before the first is used: DEPTH * ROWS loads of P in flight per lane.  The order of
    // a lane's sums is still ascending j.
    for (int j0 = threadIdx.x; j0 < N; j0 += THREADS * DEPTH) {
        double2 yj[DEPTH];
        double p[DEPTH][ROWS];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int j = j0 + u * THREADS;
            const bool in = j < N;
            yj[u] = Y[in ? j : N - 1];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) p[u][r] = in && r < rows ? P[(long long)(i0 + r) * N + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int j = j0 + u * THREADS;
            if (j >= N) break;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                if (r < rows) {   // uniform over the block
                    const double dx = yi_s[r].x - yj[u].x, dy = yi_s[r].y - yj[u].y;
                    const double w = 1.0 / (1.0 + dx * dx + dy * dy);
                    const double pw = p[u][r] * w, ww = w * w;
                    acc[r * ACC + 0] += pw * dx;
                    acc[r * ACC + 1] += pw * dy;
                    acc[r * ACC + 2] += ww * dx;
                    acc[r * ACC + 3] += ww * dy;
                    acc[r * ACC + 4] += j == i0 + r ? 0.0 : w;
                }
            }
        }
    }
    block_sum(acc, red);
#pragma unroll
    for (int k = 0; k < ROWS * ACC; ++k)   // thread k stores total k: a static register index, so nothing goes to scratch
        if (k < rows * ACC && (int)threadIdx.x == k) work[(long long)i0 * ACC + k] = acc[k];
}

__global__ __launch_bounds__(THREADS) void tsne_update_kernel(const double* __restrict__ work, int N, double alpha, double mu, double lr,
                                                              double* __restrict__ Y, double* __restrict__ V, double* __restrict__ G) {
    __shared__ double red[WAVES];
    double z[1] = {0.0};
    for (int j = threadIdx.x; j < N; j += THREADS) z[0] += work[(long long)j * ACC + 4];
    block_sum(z, red);   // the same order in every block: every block holds the same Z
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const double* a = work + (long long)i * ACC;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double g = 4.0 * (alpha * a[c] - a[2 + c] / z[0]);
        const int at = 2 * i + c;
        const double v = V[at];
        double gain = G[at];
        gain = g * v < 0.0 ? gain + 0.2 : gain * 0.8;
        gain = gain < 0.01 ? 0.01 : gain;
        const double vn = mu * v - lr * gain * g;
        G[at] = gain;
        V[at] = vn;
        Y[at] += vn;
    }
}

// ------------------------------------------------------------------------------------------------------------------ cost, placement
__global__ __launch_bounds__(THREADS) void bmap_cost_rows_kernel(const double* __restrict__ P, int N, const double2* __restrict__ Y,
                                                                 double* __restrict__ work) {
    __shared__ double red[WAVES * 3];
    const int i = blockIdx.x;
    const double2 yi = Y[i];
    double v[3] = {0.0, 0.0, 0.0};   // sum P (log P - log w), sum P, sum_{j != i} w
    for (int j = threadIdx.x; j < N; j += THREADS) {
        const double2 yj = Y[j];
        const double dx = yi.x - yj.x, dy = yi.y - yj.y;
        const double s = 1.0 + dx * dx + dy * dy;
        const double p = P[(long long)i * N + j];
        if (p > 0.0) {
            v[0] += p * (log(p) + log(s));
            v[1] += p;
        }
        if (j != i) v[2] += 1.0 / s;
    }
    block_sum(v, red);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if ((int)threadIdx.x == k) work[(long long)i * 3 + k] = v[k];
}

__global__ __launch_bounds__(THREADS) void bmap_cost_fold_kernel(const double* __restrict__ work, int N, double* __restrict__ cost) {
    __shared__ double red[WAVES * 3];
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < N; i += THREADS)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += work[(long long)i * 3 + k];
    block_sum(v, red);
    if (threadIdx.x == 0) cost[0] = v[0] + log(v[2]) * v[1];
}

__global__ __launch_bounds__(THREADS) void bmap_place_kernel(const double* __restrict__ c, int N, const double2* __restrict__ Y,
                                                             double2* __restrict__ out) {
    __shared__ double red[WAVES * 2];
    const long long t = blockIdx.x;
    double v[2] = {0.0, 0.0};
    for (int j = threadIdx.x; j < N; j += THREADS) {
        const double w = c[t * N + j];
        const double2 y = Y[j];
        v[0] += w * y.x;
        v[1] += w * y.y;
    }
    block_sum(v, red);
    if (threadIdx.x == 0) out[t] = make_double2(v[0], v[1]);
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct Range {
    const char* name;
    const void* ptr;
    long long bytes;
    int align;
};

// null, alignment and pairwise overlap of the buffers of one call; the message names the argument
int check_buffers(const char* fn, const Range* r, int count) {
    for (int a = 0; a < count; ++a) {
        if (!r[a].ptr) {
            df3d::set_error("%s: null pointer: %s", fn, r[a].name);
            return DF3D_EINVAL;
        }
        if ((uintptr_t)r[a].ptr & (uintptr_t)(r[a].align - 1)) {
            df3d::set_error("%s: %s must be %d-byte aligned", fn, r[a].name, r[a].align);
            return DF3D_EINVAL;
        }
    }
    for (int a = 0; a < count; ++a)
        for (int b = a + 1; b < count; ++b) {
            const char *pa = static_cast<const char*>(r[a].ptr), *pb = static_cast<const char*>(r[b].ptr);
            if (pa < pb + r[b].bytes && pb < pa + r[a].bytes) {
                df3d::set_error("%s: %s must not overlap %s", fn, r[b].name, r[a].name);
                return DF3D_EINVAL;
            }
        }
    return DF3D_OK;
}

#define BMAP_BUFFERS(...)                                                                   \
    do {                                                                                    \
        const Range ranges__[] = {__VA_ARGS__};                                             \
        if (const int rc__ = check_buffers(__func__, ranges__, (int)(sizeof(ranges__) / sizeof(Range)))) return rc__; \
    } while (0)

constexpr long long GRID_MAX = 0x7fffffffLL;

long long tsne_work_bytes(long long N) { return ((N * ACC * 8 + 15) / 16) * 16; }

}  // namespace

extern "C" long long df3d_bmap_work_bytes(int N) { return N < 1 || N > MAX_POINTS ? 0 : tsne_work_bytes(N); }

extern "C" int df3d_bmap_prepare(const double* S_dev, long long T, int D, double floor_, double* p_dev, double* logp_dev, double* e_dev,
                                 int* valid_dev, void* stream) {
    DF3D_CHECK_ARG(T >= 0, "T must be >= 0");
    DF3D_CHECK_ARG(D >= 1, "D must be >= 1");
    DF3D_CHECK_ARG(std::isfinite(floor_) && floor_ >= 0.0, "floor must be finite and >= 0");
    DF3D_CHECK_ARG(T <= GRID_MAX && T <= (1LL << 59) / D, "T is too large (one block per row, at most 2^31 - 1 blocks)");
    if (T == 0) return DF3D_OK;
    const long long nb = T * D * 8;
    BMAP_BUFFERS({"S", S_dev, nb, 8}, {"p", p_dev, nb, 8}, {"logp", logp_dev, nb, 8}, {"e", e_dev, T * 8, 8}, {"valid", valid_dev, T * 4, 4});
    hipLaunchKernelGGL(bmap_prepare_kernel<true>, dim3((unsigned)T), dim3(THREADS), 0, df3d::as_stream(stream), S_dev, D, floor_, p_dev, logp_dev,
                       e_dev, valid_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bmap_logs(const double* p_dev, long long T, int D, double* logp_dev, double* e_dev, void* stream) {
    DF3D_CHECK_ARG(T >= 0, "T must be >= 0");
    DF3D_CHECK_ARG(D >= 1, "D must be >= 1");
    DF3D_CHECK_ARG(T <= GRID_MAX && T <= (1LL << 59) / D, "T is too large (one block per row, at most 2^31 - 1 blocks)");
    if (T == 0) return DF3D_OK;
    const long long nb = T * D * 8;
    BMAP_BUFFERS({"p", p_dev, nb, 8}, {"logp", logp_dev, nb, 8}, {"e", e_dev, T * 8, 8});
    hipLaunchKernelGGL(bmap_prepare_kernel<false>, dim3((unsigned)T), dim3(THREADS), 0, df3d::as_stream(stream), p_dev, D, 0.0, nullptr, logp_dev,
                       e_dev, nullptr);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bmap_divergence(const double* pa_dev, const double* ea_dev, long long M, const double* lb_dev, long long N, int D,
                                    double* K_dev, void* stream) {
    DF3D_CHECK_ARG(M >= 0, "M must be >= 0");
    DF3D_CHECK_ARG(N >= 0, "N must be >= 0");
    DF3D_CHECK_ARG(D >= 1, "D must be >= 1");
    const long long by = (M + TM - 1) / TM, bx = (N + TN - 1) / TN;
    DF3D_CHECK_ARG(by <= 65535, "M is too large (the grid holds at most 65 535 tiles of 128 rows: call in row chunks)");
    DF3D_CHECK_ARG(bx <= GRID_MAX && N <= (1LL << 59) / D && (M == 0 || N <= (1LL << 59) / M), "N is too large");
    if (M == 0 || N == 0) return DF3D_OK;
    BMAP_BUFFERS({"pa", pa_dev, M * D * 8, 8}, {"ea", ea_dev, M * 8, 8}, {"K", K_dev, M * N * 8, 8});
    BMAP_BUFFERS({"lb", lb_dev, N * D * 8, 8}, {"K", K_dev, M * N * 8, 8});   // pa and lb may belong to the same set
    hipLaunchKernelGGL(bmap_divergence_kernel, dim3((unsigned)bx, (unsigned)by), dim3(THREADS), 0, df3d::as_stream(stream), pa_dev, ea_dev, M, lb_dev, N,
                       D, K_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bmap_calibrate(const double* K_dev, long long M, int N, double perplexity, double tol, double beta_max, const int* exclude_dev,
                                   double* cond_dev, double* beta_dev, int* info_dev, void* stream) {
    DF3D_CHECK_ARG(M >= 0, "M must be >= 0");
    if (N < 1 || N > MAX_POINTS) {
        df3d::set_error("%s: N must be in [1, %d] (it is %d)", __func__, MAX_POINTS, N);
        return DF3D_EINVAL;
    }
    DF3D_CHECK_ARG(std::isfinite(perplexity) && perplexity > 1.0, "perplexity must be finite and > 1");
    const int n = N - (exclude_dev ? 1 : 0);
    if (3.0 * perplexity > (double)n) {
        df3d::set_error("%s: perplexity %g needs at least %.0f points to choose from (3 perplexity <= n) and this row has %d%s: the smallest "
                        "frame count accepted is %.0f, the largest perplexity for this one %.9g",
                        __func__, perplexity, std::ceil(3.0 * perplexity), n, exclude_dev ? " (the row itself is excluded)" : "",
                        std::ceil(3.0 * perplexity) + (exclude_dev ? 1 : 0), (double)n / 3.0);
        return DF3D_EINVAL;
    }
    DF3D_CHECK_ARG(std::isfinite(tol) && tol > 0.0, "tol must be finite and > 0");
    DF3D_CHECK_ARG(std::isfinite(beta_max) && beta_max > 0.0, "beta_max must be finite and > 0");
    DF3D_CHECK_ARG(M <= GRID_MAX, "M is too large (one block per row, at most 2^31 - 1 blocks)");
    if (M == 0) return DF3D_OK;
    const long long nb = M * N * 8;
    if (exclude_dev) BMAP_BUFFERS({"exclude", exclude_dev, M * 4, 4}, {"cond", cond_dev, nb, 8}, {"beta", beta_dev, M * 8, 8}, {"info", info_dev, M * 4, 4});
    BMAP_BUFFERS({"K", K_dev, nb, 8}, {"cond", cond_dev, nb, 8}, {"beta", beta_dev, M * 8, 8}, {"info", info_dev, M * 4, 4});
    const size_t lds = sizeof(double) * (size_t)N;
    // the attribute belongs to the CURRENT device, and a process may drive several: set on every launch that needs it
    if (lds > 48 * 1024)
        DF3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bmap_calibrate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bmap_calibrate_kernel, dim3((unsigned)M), dim3(THREADS), lds, df3d::as_stream(stream), K_dev, N, std::log(perplexity), tol,
                       beta_max, exclude_dev, cond_dev, beta_dev, info_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bmap_joint(const double* cond_dev, int N, double* P_dev, void* stream) {
    if (N < 0 || N > MAX_POINTS) {
        df3d::set_error("%s: N must be in [0, %d] (it is %d)", __func__, MAX_POINTS, N);
        return DF3D_EINVAL;
    }
    if (N == 0) return DF3D_OK;
    const long long nb = (long long)N * N * 8;
    BMAP_BUFFERS({"cond", cond_dev, nb, 8}, {"P", P_dev, nb, 8});
    const unsigned tiles = (unsigned)((N + 31) / 32);
    hipLaunchKernelGGL(bmap_joint_kernel, dim3(tiles, tiles), dim3(THREADS), 0, df3d::as_stream(stream), cond_dev, N, P_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bmap_place(const double* cond_dev, long long M, int N, const double* Y_dev, double* out_dev, void* stream) {
    DF3D_CHECK_ARG(M >= 0, "M must be >= 0");
    DF3D_CHECK_ARG(N >= 1, "N must be >= 1");
    DF3D_CHECK_ARG(M <= GRID_MAX && M <= (1LL << 59) / N, "M is too large (one block per row, at most 2^31 - 1 blocks)");
    if (M == 0) return DF3D_OK;
    BMAP_BUFFERS({"cond", cond_dev, M * N * 8, 8}, {"Y", Y_dev, (long long)N * 16, 16}, {"out", out_dev, M * 16, 16});
    hipLaunchKernelGGL(bmap_place_kernel, dim3((unsigned)M), dim3(THREADS), 0, df3d::as_stream(stream), cond_dev, N,
                       reinterpret_cast<const double2*>(Y_dev), reinterpret_cast<double2*>(out_dev));
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bmap_cost(const double* P_dev, int N, const double* Y_dev, double* cost_dev, void* work_dev, long long work_len_bytes,
                              void* stream) {
    if (N < 1 || N > MAX_POINTS) {
        df3d::set_error("%s: N must be in [1, %d] (it is %d)", __func__, MAX_POINTS, N);
        return DF3D_EINVAL;
    }
    DF3D_CHECK_ARG(work_len_bytes >= tsne_work_bytes(N), "work buffer too small (df3d_bmap_work_bytes)");
    BMAP_BUFFERS({"P", P_dev, (long long)N * N * 8, 8}, {"Y", Y_dev, (long long)N * 16, 16}, {"cost", cost_dev, 8, 8},
                 {"work", work_dev, tsne_work_bytes(N), 16});
    hipLaunchKernelGGL(bmap_cost_rows_kernel, dim3((unsigned)N), dim3(THREADS), 0, df3d::as_stream(stream), P_dev, N,
                       reinterpret_cast<const double2*>(Y_dev), static_cast<double*>(work_dev));
    DF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(bmap_cost_fold_kernel, dim3(1), dim3(THREADS), 0, df3d::as_stream(stream), static_cast<const double*>(work_dev), N, cost_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_tsne_run(const double* P_dev, int N, double* Y_dev, double* V_dev, double* G_dev, int first_iter, int num_iters, double lr,
                             void* work_dev, long long work_len_bytes, void* stream) {
    if (N < 1 || N > MAX_POINTS) {
        df3d::set_error("%s: N must be in [1, %d] (it is %d)", __func__, MAX_POINTS, N);
        return DF3D_EINVAL;
    }
    DF3D_CHECK_ARG(first_iter >= 0, "first_iter must be >= 0");
    DF3D_CHECK_ARG(num_iters >= 0 && num_iters <= 0x7fffffff - first_iter, "num_iters must be >= 0 and first_iter + num_iters below 2^31");
    DF3D_CHECK_ARG(std::isfinite(lr) && lr > 0.0, "lr must be finite and > 0");
    if (num_iters == 0) return DF3D_OK;
    DF3D_CHECK_ARG(work_len_bytes >= tsne_work_bytes(N), "work buffer too small (df3d_bmap_work_bytes)");
    const long long ny = (long long)N * 16;
    BMAP_BUFFERS({"P", P_dev, (long long)N * N * 8, 8}, {"Y", Y_dev, ny, 16}, {"V", V_dev, ny, 8}, {"G", G_dev, ny, 8},
                 {"work", work_dev, tsne_work_bytes(N), 16});
    const unsigned gblocks = (unsigned)((N + ROWS - 1) / ROWS), ublocks = (unsigned)((N + THREADS - 1) / THREADS);
    for (int k = first_iter; k < first_iter + num_iters; ++k) {
        const bool early = k < EXAGGERATION_ITERS;   // alpha and mu follow the absolute iteration index
        hipLaunchKernelGGL(tsne_gradient_kernel, dim3(gblocks), dim3(THREADS), 0, df3d::as_stream(stream), P_dev, N,
                           reinterpret_cast<const double2*>(Y_dev), static_cast<double*>(work_dev));
        hipLaunchKernelGGL(tsne_update_kernel, dim3(ublocks), dim3(THREADS), 0, df3d::as_stream(stream), static_cast<const double*>(work_dev), N,
                           early ? 12.0 : 1.0, early ? 0.5 : 0.8, lr, Y_dev, V_dev, G_dev);
    }
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
