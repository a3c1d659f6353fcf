// a14 segmentation of the behaviour map (the model is this project's own specification, defined in float64 by
// tests/behaviour_segment_oracle.py): a Gaussian density of the map on a square grid, steepest-ascent watershed regions round its
// peaks, a label per frame and the ethogram.  Every stage is its own entry.  No floating-point atomics, every floating-point sum
// in a fixed order, every integer output exact.
//
// bseg_bounds_kernel: one block; min and max per axis and the count of the valid rows (both entries finite) -> 5 doubles.
// bseg_density_kernel: rho is separable, sum_t A[r, t] B[t, q] with A[r, t] = exp(-(gy_r - y_t)^2 / 2 sigma^2) and B likewise in x: a
//     [G x T] . [T x G] float64 product whose operands are made on the fly.  A block owns a 64 x 64 tile of rho and one slice of
//     SLICE frames (a constant: the bits do not depend on the machine).  Per chunk of CHUNK frames it writes A and B into LDS
//     (128 exponentials per frame for 4 096 multiply-adds; an invalid frame, a frame past the slice and a cell past the grid are
//     written as 0) and each of the four waves carries a 32 x 32 sub-tile as 2 x 2 v_mfma_f64_16x16x4_f64 accumulators.  The partial
//     tile goes to the workspace [S, G, G].
// bseg_density_fold_kernel: adds the S slices in index order and divides by M 2 pi sigma^2.
// bseg_max_kernel: one block, max rho in a fixed order.  bseg_ascent_kernel: every cell's pointer to the 8-neighbour with the
//     largest key (rho, -index), or to itself (a root).  bseg_jump_kernel: p <- p[p] between two buffers, ceil(log2 G^2) launches.
// bseg_scan_*: an int32 exclusive scan of any length in three phases (sums of blocks of 256, one block scans the sums, add); it
//     numbers the kept roots and the bout starts.
// bseg_keep_kernel, bseg_regions_kernel: the kept roots, the region of every cell and the roots' cells.
// bseg_labels_kernel: the cell of every frame.  bseg_starts_kernel, bseg_bout_starts_kernel, bseg_bouts_kernel: the runs of equal
//     labels; bseg_counts_kernel: occupancy and transitions by integer atomics (exact whatever the order).
#include <cmath>
#include <cstdint>

#include "common.h"

// Built with -ffp-contract=off (build.py): the grid coordinates, the cell of a frame and the peak threshold are the oracle's IEEE
// operations one by one, never a fused multiply-add.

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / df3d::WAVE;
constexpr int G_MIN = 2, G_MAX = 1024;
constexpr int TILE = 64;        // a block's tile of rho
constexpr int CHUNK = 32;       // frames whose exponentials sit in LDS together
constexpr int STRIDE = 80;      // doubles per frame row of LDS: 160 dwords, so the four frames one MFMA operand reads start 32 banks apart
constexpr int SLICE = 2048;     // frames per block: a constant, never the CU count
constexpr long long HEADER = 64;   // bytes in front of every workspace layout: the bounds' five doubles, or max rho
constexpr long long GRID_MAX = 0x7fffffffLL;
constexpr double TWO_PI = 6.283185307179586476925286766559;

typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool valid_row(double2 y) { return isfinite(y.x) && isfinite(y.y); }

// ------------------------------------------------------------------------------------------------------------------ bounds
__global__ __launch_bounds__(THREADS) void bseg_bounds_kernel(const double2* __restrict__ Y, long long T, double* __restrict__ out) {
    __shared__ double red[WAVES][5];
    double v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0};   // min x, max x, min y, max y, count (exact below 2^53)
    for (long long t = threadIdx.x; t < T; t += THREADS) {
        const double2 y = Y[t];
        if (valid_row(y)) {
            v[0] = fmin(v[0], y.x);
            v[1] = fmax(v[1], y.x);
            v[2] = fmin(v[2], y.y);
            v[3] = fmax(v[3], y.y);
            v[4] += 1.0;
        }
    }
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
#pragma unroll
    for (int o = df3d::WAVE / 2; o > 0; o >>= 1) {
        v[0] = fmin(v[0], __shfl_down(v[0], o));
        v[1] = fmax(v[1], __shfl_down(v[1], o));
        v[2] = fmin(v[2], __shfl_down(v[2], o));
        v[3] = fmax(v[3], __shfl_down(v[3], o));
        v[4] += __shfl_down(v[4], o);
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            v[0] = fmin(v[0], red[w][0]);
            v[1] = fmax(v[1], red[w][1]);
            v[2] = fmin(v[2], red[w][2]);
            v[3] = fmax(v[3], red[w][3]);
            v[4] += red[w][4];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) out[k] = v[k];
    }
}

// ------------------------------------------------------------------------------------------------------------------ density
__global__ __launch_bounds__(THREADS) void bseg_density_kernel(const double2* __restrict__ Y, long long T, double x0, double y0, double h, int G,
                                                               double two_s2, double* __restrict__ part) {
    __shared__ double As[CHUNK][STRIDE];   // As[t][r]: the rows (y) of the tile
    __shared__ double Bs[CHUNK][STRIDE];   // Bs[t][q]: its columns (x)
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
    const int r0 = blockIdx.y * TILE, q0 = blockIdx.x * TILE;
    const long long t0 = (long long)blockIdx.z * SLICE;
    const long long t1 = t0 + SLICE < T ? t0 + SLICE : T;
    // the fill: waves 0 and 2 write A, waves 1 and 3 write B; lane = the cell along the tile; a wave takes every other frame pair
    const bool fill_b = wave & 1;
    const int cell = (fill_b ? q0 : r0) + lane;
    const double g = (fill_b ? x0 : y0) + ((double)cell + 0.5) * h;   // the oracle's grid coordinate, operation by operation
    const bool cell_in = cell < G;
    double (*dst)[STRIDE] = fill_b ? Bs : As;
    // the product: wave w owns rows wr .. wr + 31 and columns wc .. wc + 31 of the tile
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int m = lane & 15, k4 = lane >> 4;
    double4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (long long c0 = t0; c0 < t1; c0 += CHUNK) {
#pragma unroll 4
        for (int f = (wave >> 1); f < CHUNK; f += 2) {
            const long long t = c0 + f;
            double e = 0.0;
            if (t < t1) {   // uniform over the wave
                const double2 y = Y[t];
                if (valid_row(y) && cell_in) {   // selection, never arithmetic on a NaN
                    const double d = g - (fill_b ? y.x : y.y);
                    e = exp(-(d * d) / two_s2);
                }
            }
            dst[f][lane] = e;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CHUNK; kk += 4) {
            // A and B as in the f32 16 x 16 x 4 form: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]
            const double a0 = As[kk + k4][wr + m], a1 = As[kk + k4][wr + 16 + m];
            const double b0 = Bs[kk + k4][wc + m], b1 = Bs[kk + k4][wc + 16 + m];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
    double* out = part + (long long)blockIdx.z * G * G;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = r0 + wr + 16 * i + k4 + 4 * reg, q = q0 + wc + 16 * j + m;
                if (r < G && q < G) out[(long long)r * G + q] = acc[i][j][reg];
            }
}

__global__ __launch_bounds__(THREADS) void bseg_density_fold_kernel(const double* __restrict__ part, int S, int G, const double* __restrict__ bounds,
                                                                    double sigma, double* __restrict__ rho) {
    const int n = G * G, i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    double s = part[i];
    for (int k = 1; k < S; ++k) s += part[(long long)k * n + i];
    const double M = bounds[4];
    rho[i] = M > 0.0 ? s / (M * TWO_PI * (sigma * sigma)) : 0.0;
}

// ------------------------------------------------------------------------------------------------------------------ watershed
__global__ __launch_bounds__(THREADS) void bseg_max_kernel(const double* __restrict__ rho, int n, double* __restrict__ out) {
    __shared__ double red[WAVES];
    double v = -INFINITY;
    for (int i = threadIdx.x; i < n; i += THREADS) v = fmax(v, rho[i]);
    const int lane = threadIdx.x & (df3d::WAVE - 1), wave = threadIdx.x / df3d::WAVE;
#pragma unroll
    for (int o = df3d::WAVE / 2; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o));
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v = fmax(v, red[w]);
        out[0] = v;
    }
}

// key(a) > key(b) for the key (rho, -index)
__device__ __forceinline__ bool key_above(double ra, int ia, double rb, int ib) { return ra > rb || (ra == rb && ia < ib); }

__global__ __launch_bounds__(THREADS) void bseg_ascent_kernel(const double* __restrict__ rho, int G, int* __restrict__ ptr) {
    const int n = G * G, i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = i / G, q = i - r * G;
    double best = rho[i];
    int at = i;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
        for (int dq = -1; dq <= 1; ++dq) {
            const int rr = r + dr, qq = q + dq;
            if ((dr || dq) && rr >= 0 && rr < G && qq >= 0 && qq < G) {
                const int j = rr * G + qq;
                const double v = rho[j];
                if (key_above(v, j, best, at)) {
                    best = v;
                    at = j;
                }
            }
        }
    ptr[i] = at;
}

__global__ __launch_bounds__(THREADS) void bseg_jump_kernel(const int* __restrict__ src, int n, int* __restrict__ dst) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < n) dst[i] = src[src[i]];
}

__global__ __launch_bounds__(THREADS) void bseg_keep_kernel(const double* __restrict__ rho, const int* __restrict__ root, int n, double min_peak,
                                                            const double* __restrict__ max_rho, int* __restrict__ keep) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const double v = rho[i];
    keep[i] = root[i] == i && v > 0.0 && v >= min_peak * max_rho[0] ? 1 : 0;
}

// number: the exclusive scan of keep; total[0] = R.  root_cells [n]: the first R entries are the kept roots, the others -1.
__global__ __launch_bounds__(THREADS) void bseg_regions_kernel(const int* __restrict__ root, const int* __restrict__ keep, const int* __restrict__ number,
                                                               const int* __restrict__ total, int n, int* __restrict__ regions,
                                                               int* __restrict__ root_cells) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int at = root[i];
    regions[i] = keep[at] ? number[at] + 1 : 0;
    if (keep[i]) root_cells[number[i]] = i;
    if (i >= total[0]) root_cells[i] = -1;
}

// ------------------------------------------------------------------------------------------------------------------ the scan
// The exclusive scan of v over the block, the block's sum in `total`.  lds: THREADS ints.
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds, int& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    int s = v;
    for (int o = 1; o < THREADS; o <<= 1) {
        const int add = t >= o ? lds[t - o] : 0;
        __syncthreads();
        s += add;
        lds[t] = s;
        __syncthreads();
    }
    total = lds[THREADS - 1];
    __syncthreads();   // the next call may write lds
    return s - v;
}

__global__ __launch_bounds__(THREADS) void bseg_scan_sums_kernel(const int* __restrict__ in, long long n, int* __restrict__ sums) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int total;
    block_exclusive_scan(i < n ? in[i] : 0, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums -> their exclusive scan, in place, 256 at a time with a carry; total[0] = the sum of all
__global__ __launch_bounds__(THREADS) void bseg_scan_offsets_kernel(int* __restrict__ sums, long long nb, int* __restrict__ total) {
    __shared__ int lds[THREADS];
    int carry = 0;
    for (long long b0 = 0; b0 < nb; b0 += THREADS) {
        const long long b = b0 + threadIdx.x;
        int chunk;
        const int ex = block_exclusive_scan(b < nb ? sums[b] : 0, lds, chunk);
        if (b < nb) sums[b] = carry + ex;
        carry += chunk;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ __launch_bounds__(THREADS) void bseg_scan_add_kernel(const int* __restrict__ in, long long n, const int* __restrict__ sums,
                                                                int* __restrict__ out) {
    __shared__ int lds[THREADS];
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    int total;
    const int ex = block_exclusive_scan(i < n ? in[i] : 0, lds, total);
    if (i < n) out[i] = sums[blockIdx.x] + ex;
}

// ------------------------------------------------------------------------------------------------------------------ labels, ethogram
__device__ __forceinline__ int cell_of(double v, double origin, double h, int G) {
    double c = floor((v - origin) / h);
    c = c < 0.0 ? 0.0 : c;
    c = c > (double)(G - 1) ? (double)(G - 1) : c;
    return (int)c;
}

__global__ __launch_bounds__(THREADS) void bseg_labels_kernel(const double2* __restrict__ Y, long long T, double x0, double y0, double h, int G,
                                                              const int* __restrict__ regions, int* __restrict__ labels) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T) return;
    const double2 y = Y[t];
    labels[t] = valid_row(y) ? regions[cell_of(y.y, y0, h, G) * G + cell_of(y.x, x0, h, G)] : -1;
}

__global__ __launch_bounds__(THREADS) void bseg_starts_kernel(const int* __restrict__ labels, long long T, int* __restrict__ flag) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t < T) flag[t] = t == 0 || labels[t] != labels[t - 1] ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void bseg_bout_starts_kernel(const int* __restrict__ flag, const int* __restrict__ number, long long T,
                                                                   int* __restrict__ starts) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t < T && flag[t]) starts[number[t]] = (int)t;
}

// bouts [T, 3]: row b < B is (label, start, length); the rows from B on are zero
__global__ __launch_bounds__(THREADS) void bseg_bouts_kernel(const int* __restrict__ labels, const int* __restrict__ starts, const int* __restrict__ total,
                                                             long long T, long long* __restrict__ bouts) {
    const long long b = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (b >= T) return;
    const int B = total[0];
    long long row[3] = {0, 0, 0};
    if (b < B) {
        const long long s = starts[b], e = b + 1 < B ? (long long)starts[b + 1] : T;
        row[0] = labels[s];
        row[1] = s;
        row[2] = e - s;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) bouts[b * 3 + k] = row[k];
}

__global__ __launch_bounds__(THREADS) void bseg_zero_kernel(unsigned long long* __restrict__ p, long long n) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) p[i] = 0ULL;
}

// A block counts COUNT_FRAMES frames.  Up to COUNT_LOCAL labels (R + 1) it counts in LDS first and adds its non-zero counts to the
// tables once: a recording visits few labels, and one global atomic per frame would queue on a handful of addresses.  A label
// outside [-1, R] is counted nowhere: nothing is written out of bounds whatever the input.
constexpr int COUNT_LOCAL = 32, COUNT_PER_THREAD = 8, COUNT_FRAMES = THREADS * COUNT_PER_THREAD;

__global__ __launch_bounds__(THREADS) void bseg_counts_kernel(const int* __restrict__ labels, long long T, int R, unsigned long long* __restrict__ occupancy,
                                                              unsigned long long* __restrict__ transitions) {
    __shared__ unsigned int local[COUNT_LOCAL * COUNT_LOCAL + COUNT_LOCAL];   // the transitions, then the occupancy
    const int R1 = R + 1, cells = R1 * R1;
    const bool in_lds = R1 <= COUNT_LOCAL;   // uniform
    if (in_lds) {
        for (int k = threadIdx.x; k < cells + R1; k += THREADS) local[k] = 0u;
        __syncthreads();
    }
    const long long t0 = (long long)blockIdx.x * COUNT_FRAMES;
#pragma unroll
    for (int i = 0; i < COUNT_PER_THREAD; ++i) {
        const long long t = t0 + i * THREADS + threadIdx.x;
        if (t >= T) break;
        const int a = labels[t];
        if (a < 0 || a > R) continue;
        const int b = t + 1 < T ? labels[t + 1] : -1;
        const bool pair = b >= 0 && b <= R && b != a;
        if (in_lds) {
            atomicAdd(&local[cells + a], 1u);
            if (pair) atomicAdd(&local[a * R1 + b], 1u);
        } else {
            atomicAdd(&occupancy[a], 1ULL);
            if (pair) atomicAdd(&transitions[(long long)a * R1 + b], 1ULL);
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < cells + R1; k += THREADS) {
            const unsigned int c = local[k];
            if (c) atomicAdd(k < cells ? &transitions[k] : &occupancy[k - cells], (unsigned long long)c);
        }
    }
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

#define BSEG_BUFFERS(...)                                                                   \
    do {                                                                                    \
        const Range ranges__[] = {__VA_ARGS__};                                             \
        if (const int rc__ = check_buffers(__func__, ranges__, (int)(sizeof(ranges__) / sizeof(Range)))) return rc__; \
    } while (0)

#define BSEG_CHECK_GRID(G)                                                                             \
    do {                                                                                               \
        if ((G) < G_MIN || (G) > G_MAX) {                                                              \
            df3d::set_error("%s: G must be in [%d, %d] (it is %d)", __func__, G_MIN, G_MAX, (int)(G)); \
            return DF3D_EINVAL;                                                                        \
        }                                                                                              \
    } while (0)

long long round64(long long b) { return (b + 63) / 64 * 64; }
long long blocks_of(long long n) { return (n + THREADS - 1) / THREADS; }
long long slices_of(long long T) { return T > 0 ? (T + SLICE - 1) / SLICE : 1; }
constexpr long long T_MAX = 65535LL * SLICE;   // the density's grid holds at most 65 535 slices

// the three workspace layouts, each behind a header of HEADER bytes
long long density_bytes(long long T, int G) { return HEADER + slices_of(T) * G * G * 8; }
// the scan's users: three int32 arrays of n (the two jump buffers and the roots' numbers; the flags, their numbers and the bout starts)
// and the block sums
long long scan_user_bytes(long long n) { return HEADER + 3 * round64(n * 4) + round64(blocks_of(n) * 4); }

unsigned grid_of(long long n) { return (unsigned)blocks_of(n); }

// out = the exclusive scan of in [n], total[0] = its sum
void launch_scan(const int* in, long long n, int* sums, int* total, int* out, hipStream_t st) {
    const unsigned nb = grid_of(n);
    hipLaunchKernelGGL(bseg_scan_sums_kernel, dim3(nb), dim3(THREADS), 0, st, in, n, sums);
    hipLaunchKernelGGL(bseg_scan_offsets_kernel, dim3(1), dim3(THREADS), 0, st, sums, (long long)nb, total);
    hipLaunchKernelGGL(bseg_scan_add_kernel, dim3(nb), dim3(THREADS), 0, st, in, n, sums, out);
}

}  // namespace

extern "C" long long df3d_bseg_work_bytes(long long T, int G) {
    if (T < 0 || T > T_MAX || G < G_MIN || G > G_MAX) return 0;
    const long long a = density_bytes(T, G), b = scan_user_bytes((long long)G * G), c = scan_user_bytes(T);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

extern "C" int df3d_bseg_bounds(const double* Y_dev, long long T, double* bounds_dev, void* stream) {
    DF3D_CHECK_ARG(T >= 0 && T <= T_MAX, "T must be in [0, 65 535 * 2 048]");
    if (T == 0) return DF3D_OK;
    BSEG_BUFFERS({"Y", Y_dev, T * 16, 16}, {"bounds", bounds_dev, 40, 8});
    hipLaunchKernelGGL(bseg_bounds_kernel, dim3(1), dim3(THREADS), 0, df3d::as_stream(stream), reinterpret_cast<const double2*>(Y_dev), T, bounds_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bseg_density(const double* Y_dev, long long T, double x0, double y0, double h, int G, double sigma, double* rho_dev,
                                 void* work_dev, long long work_len_bytes, void* stream) {
    DF3D_CHECK_ARG(T >= 0 && T <= T_MAX, "T must be in [0, 65 535 * 2 048]");
    BSEG_CHECK_GRID(G);
    DF3D_CHECK_ARG(std::isfinite(x0) && std::isfinite(y0), "x0 and y0 must be finite");
    DF3D_CHECK_ARG(std::isfinite(h) && h > 0.0, "h must be finite and > 0");
    DF3D_CHECK_ARG(std::isfinite(sigma) && sigma > 0.0 && std::isfinite(sigma * sigma) && std::isfinite(1.0 / (sigma * sigma)),
                   "sigma must be finite and > 0 (and so must its square and that square's inverse)");
    if (T == 0) return DF3D_OK;
    const long long need = density_bytes(T, G);
    DF3D_CHECK_ARG(work_len_bytes >= need, "work buffer too small (df3d_bseg_work_bytes)");
    BSEG_BUFFERS({"Y", Y_dev, T * 16, 16}, {"rho", rho_dev, (long long)G * G * 8, 8}, {"work", work_dev, need, 16});
    hipStream_t st = df3d::as_stream(stream);
    double* bounds = static_cast<double*>(work_dev);
    double* part = reinterpret_cast<double*>(static_cast<char*>(work_dev) + HEADER);
    const double2* Y = reinterpret_cast<const double2*>(Y_dev);
    const int S = (int)slices_of(T);
    const unsigned tiles = (unsigned)((G + TILE - 1) / TILE);
    hipLaunchKernelGGL(bseg_bounds_kernel, dim3(1), dim3(THREADS), 0, st, Y, T, bounds);
    hipLaunchKernelGGL(bseg_density_kernel, dim3(tiles, tiles, (unsigned)S), dim3(THREADS), 0, st, Y, T, x0, y0, h, G, 2.0 * (sigma * sigma), part);
    hipLaunchKernelGGL(bseg_density_fold_kernel, dim3(grid_of((long long)G * G)), dim3(THREADS), 0, st, part, S, G, bounds, sigma, rho_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bseg_watershed(const double* rho_dev, int G, double min_peak, int* regions_dev, int* num_regions_dev, int* root_cells_dev,
                                   void* work_dev, long long work_len_bytes, void* stream) {
    BSEG_CHECK_GRID(G);
    DF3D_CHECK_ARG(min_peak >= 0.0 && min_peak <= 1.0, "min_peak must be in [0, 1]");
    const long long n = (long long)G * G, need = scan_user_bytes(n);
    DF3D_CHECK_ARG(work_len_bytes >= need, "work buffer too small (df3d_bseg_work_bytes)");
    BSEG_BUFFERS({"rho", rho_dev, n * 8, 8}, {"regions", regions_dev, n * 4, 4}, {"num_regions", num_regions_dev, 4, 4},
                 {"root_cells", root_cells_dev, n * 4, 4}, {"work", work_dev, need, 16});
    hipStream_t st = df3d::as_stream(stream);
    char* w = static_cast<char*>(work_dev);
    double* max_rho = reinterpret_cast<double*>(w);
    int* pa = reinterpret_cast<int*>(w + HEADER);
    int* pb = reinterpret_cast<int*>(w + HEADER + round64(n * 4));
    int* number = reinterpret_cast<int*>(w + HEADER + 2 * round64(n * 4));
    int* sums = reinterpret_cast<int*>(w + HEADER + 3 * round64(n * 4));
    const unsigned nb = grid_of(n);
    hipLaunchKernelGGL(bseg_max_kernel, dim3(1), dim3(THREADS), 0, st, rho_dev, (int)n, max_rho);
    hipLaunchKernelGGL(bseg_ascent_kernel, dim3(nb), dim3(THREADS), 0, st, rho_dev, G, pa);
    int rounds = 0;
    while ((1LL << rounds) < n) ++rounds;   // ceil(log2 G^2): a chain has at most G^2 - 1 links
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(bseg_jump_kernel, dim3(nb), dim3(THREADS), 0, st, pa, (int)n, pb);
        int* swap = pa;
        pa = pb;
        pb = swap;
    }
    int* keep = pb;   // pa holds every cell's root; the other jump buffer is free
    hipLaunchKernelGGL(bseg_keep_kernel, dim3(nb), dim3(THREADS), 0, st, rho_dev, pa, (int)n, min_peak, max_rho, keep);
    launch_scan(keep, n, sums, num_regions_dev, number, st);
    hipLaunchKernelGGL(bseg_regions_kernel, dim3(nb), dim3(THREADS), 0, st, pa, keep, number, num_regions_dev, (int)n, regions_dev, root_cells_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bseg_labels(const double* Y_dev, long long T, double x0, double y0, double h, int G, const int* regions_dev, int* labels_dev,
                                void* stream) {
    DF3D_CHECK_ARG(T >= 0 && T <= GRID_MAX, "T must be in [0, 2^31 - 1]");
    BSEG_CHECK_GRID(G);
    DF3D_CHECK_ARG(std::isfinite(x0) && std::isfinite(y0), "x0 and y0 must be finite");
    DF3D_CHECK_ARG(std::isfinite(h) && h > 0.0, "h must be finite and > 0");
    if (T == 0) return DF3D_OK;
    BSEG_BUFFERS({"Y", Y_dev, T * 16, 16}, {"regions", regions_dev, (long long)G * G * 4, 4}, {"labels", labels_dev, T * 4, 4});
    hipLaunchKernelGGL(bseg_labels_kernel, dim3(grid_of(T)), dim3(THREADS), 0, df3d::as_stream(stream), reinterpret_cast<const double2*>(Y_dev), T, x0, y0,
                       h, G, regions_dev, labels_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_bseg_bouts(const int* labels_dev, long long T, int num_regions, long long* bouts_dev, int* num_bouts_dev, long long* occupancy_dev,
                               long long* transitions_dev, void* work_dev, long long work_len_bytes, void* stream) {
    DF3D_CHECK_ARG(T >= 0 && T <= GRID_MAX, "T must be in [0, 2^31 - 1]");
    DF3D_CHECK_ARG(num_regions >= 0 && num_regions <= 32767, "num_regions must be in [0, 32 767] (the transition table holds (R + 1)^2 counts)");
    if (T == 0) return DF3D_OK;
    const long long need = scan_user_bytes(T), R1 = (long long)num_regions + 1;
    DF3D_CHECK_ARG(work_len_bytes >= need, "work buffer too small (df3d_bseg_work_bytes)");
    BSEG_BUFFERS({"labels", labels_dev, T * 4, 4}, {"bouts", bouts_dev, T * 24, 8}, {"num_bouts", num_bouts_dev, 4, 4},
                 {"occupancy", occupancy_dev, R1 * 8, 8}, {"transitions", transitions_dev, R1 * R1 * 8, 8}, {"work", work_dev, need, 16});
    hipStream_t st = df3d::as_stream(stream);
    char* w = static_cast<char*>(work_dev);
    int* flag = reinterpret_cast<int*>(w + HEADER);
    int* number = reinterpret_cast<int*>(w + HEADER + round64(T * 4));
    int* starts = reinterpret_cast<int*>(w + HEADER + 2 * round64(T * 4));
    int* sums = reinterpret_cast<int*>(w + HEADER + 3 * round64(T * 4));
    const unsigned nb = grid_of(T);
    hipLaunchKernelGGL(bseg_starts_kernel, dim3(nb), dim3(THREADS), 0, st, labels_dev, T, flag);
    launch_scan(flag, T, sums, num_bouts_dev, number, st);
    hipLaunchKernelGGL(bseg_bout_starts_kernel, dim3(nb), dim3(THREADS), 0, st, flag, number, T, starts);
    hipLaunchKernelGGL(bseg_bouts_kernel, dim3(nb), dim3(THREADS), 0, st, labels_dev, starts, num_bouts_dev, T, bouts_dev);
    unsigned long long* occ = reinterpret_cast<unsigned long long*>(occupancy_dev);
    unsigned long long* tr = reinterpret_cast<unsigned long long*>(transitions_dev);
    hipLaunchKernelGGL(bseg_zero_kernel, dim3(grid_of(R1)), dim3(THREADS), 0, st, occ, R1);
    hipLaunchKernelGGL(bseg_zero_kernel, dim3(grid_of(R1 * R1)), dim3(THREADS), 0, st, tr, R1 * R1);
    hipLaunchKernelGGL(bseg_counts_kernel, dim3((unsigned)((T + COUNT_FRAMES - 1) / COUNT_FRAMES)), dim3(THREADS), 0, st, labels_dev, T, num_regions, occ,
                       tr);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
