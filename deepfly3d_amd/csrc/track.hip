// a18 tracking of the 2-D detections through time (the model is this project's own specification, defined in
// float64 / int64 by tests/track_oracle.py): for every chain (camera, network joint) the sequence of heat-map peaks that is jointly best
// over the whole recording, an exact Viterbi solve.  Every cost is quantised once to an int64 multiple of 2^-20 and sums saturate at
// INF = 2^61, so (min, +) is exactly associative and any blocking over time gives the serial recurrence's integers.  No atomics: two
// runs give the same bits.  No kernel waits on another block of its grid.
//
// A frame has S = 16 states (the K slots, padded with INF).  Block b of a chain holds the frames [b B, min(T, (b + 1) B)).
// track_block_kernel<true>:  one workgroup per (chain, block), lane (s, k): the block's transfer matrix M_b [16, 16], the cost from state
//     s of the frame before the block (its own unary cost left out) to state k of the block's last frame.  Frame 0 has no pair cost.
// track_carry_kernel:        16 lanes per chain, serial over the blocks: in_b = the exact cost vector of the frame before block b
//     (in_0 = (0, INF, ...)), in_{b+1}(k) = min_s in_b(s) + M_b(s, k); then the minimum of the last vector and its lowest state.
// track_block_kernel<false>: one workgroup per (chain, block): the forward pass from in_b, lanes 0 .. 15; every frame's back-pointers
//     (the lowest minimising predecessor, one byte per state) and the block's map from exit state to entry state.
// track_exit_kernel:         one lane per chain, serial over the blocks from the last: the state every block is left in.
// track_trace_kernel:        one workgroup per (chain, block): the back-pointers 256 frames at a time in LDS, lane 0 follows them.
// The pair tables of 16 frames are formed together, one entry per lane and frame, and held in LDS (both block kernels).
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "common.h"

// Built with -ffp-contract=off (build.py): every cost is the oracle's float64 operations one by one, rounded once by rint.

namespace {

constexpr int S = 16;               // states per frame
constexpr int THREADS = S * S;      // lane (s, k) = (tid / 16, tid % 16)
constexpr int CHUNK = 16;           // frames whose costs are formed together
constexpr int RING = 2 * CHUNK;     // slot data of the frames (t - t0 + 1) mod RING: a chunk and the frame before it stay readable
constexpr int TRACE = 256;          // frames of back-pointers in LDS at a time
constexpr long long INF = 1LL << 61;   // INF + INF fits
constexpr double SCALE = 1048576.0;    // 2^20
constexpr int K_MAX = 16, BLOCK_MAX = 4096;
constexpr double W_MAX = 1024.0;
constexpr long long CHAINS_MAX = 1LL << 20, CHAIN_FRAMES_MAX = 1LL << 36;
constexpr int VALID = 1, PLACEHOLDER = 2;

struct Params {
    const int* count;
    const float* pts;
    const float* val;
    long long T, B, nb;
    int J, K;
    double H, W, tt, wm, wv;
};

struct Slot {
    double r, c;
    long long u;
    int flag;
};

struct Costs {
    double r[RING][S], c[RING][S];   // pixels of a slot
    long long u[RING][S];            // its quantised unary cost
    int flag[RING][S];
    int d[CHUNK][S * S];             // d[f][k' * 16 + k]: the pair cost of frame tc + f, at most 1024 2^20 = 2^30
};

__device__ __forceinline__ long long sat_add(long long a, long long b) {
    const long long s = a + b;
    return s < INF ? s : INF;
}

__device__ __forceinline__ long long quantise(double x) { return (long long)rint(x * SCALE); }

// Slot k of frame t of chain (c, j), by the 16 lanes of one row of a wave (every lane of the wave calls this).  `in`: the frame exists.
__device__ __forceinline__ Slot load_slot(const Params& p, int c, int j, long long t, int k, bool in) {
    float v = 0.0f, pr = 0.0f, pc = 0.0f;
    int cnt = 0;
    if (in) cnt = p.count[((size_t)c * p.T + t) * p.J + j];
    if (in && k < p.K) {
        const size_t at = (((size_t)c * p.T + t) * p.J + j) * p.K + k;
        v = p.val[at];
        pr = p.pts[2 * at];
        pc = p.pts[2 * at + 1];
    }
    const bool ok = in && k < p.K && k < cnt && isfinite(v) && isfinite(pr) && isfinite(pc);
    const unsigned row = (unsigned)(__ballot(ok) >> (threadIdx.x & 48)) & 0xffffu;
    float best = ok ? v : -INFINITY;
#pragma unroll
    for (int o = S / 2; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, S));
    Slot s = {0.0, 0.0, INF, 0};
    if (!in) return s;
    if (row == 0) {   // a placeholder frame: slot 0 alone
        if (k == 0) s = {0.0, 0.0, 0, VALID | PLACEHOLDER};
        return s;
    }
    if (ok) {
        const double gap = (double)best - (double)v;
        s = {(double)pr * p.H, (double)pc * p.W, quantise(p.wv * (gap < 1.0 ? gap : 1.0)), VALID};
    }
    return s;
}

// The slots of frames [tc, tc + nf) into the ring, and their pair tables into L.d.  Ends with a barrier.
__device__ __forceinline__ void chunk_costs(const Params& p, int c, int j, long long t0, long long tc, int nf, Costs& L) {
    const int hi = threadIdx.x >> 4, lo = threadIdx.x & 15;
    if (tc == t0) {   // the frame before the block (none before frame 0: an empty slot)
        const Slot s = load_slot(p, c, j, t0 - 1, lo, hi == 0 && t0 > 0);
        if (hi == 0) L.r[0][lo] = s.r, L.c[0][lo] = s.c, L.u[0][lo] = s.u, L.flag[0][lo] = s.flag;
    }
    {
        const Slot s = load_slot(p, c, j, tc + hi, lo, hi < nf);
        const int pos = (int)((tc - t0 + hi + 1) & (RING - 1));
        if (hi < nf) L.r[pos][lo] = s.r, L.c[pos][lo] = s.c, L.u[pos][lo] = s.u, L.flag[pos][lo] = s.flag;
    }
    __syncthreads();
    const long long qm = quantise(p.wm);
    for (int f = 0; f < nf; ++f) {   // lane (k', k)
        const int p0 = (int)((tc - t0 + f) & (RING - 1)), p1 = (p0 + 1) & (RING - 1);
        const int f0 = L.flag[p0][hi], f1 = L.flag[p1][lo];
        long long q = 0;
        if (tc + f > 0 && (f0 & f1 & VALID)) {
            if ((f0 | f1) & PLACEHOLDER) {
                q = qm;
            } else {
                const double dr = L.r[p1][lo] - L.r[p0][hi], dc = L.c[p1][lo] - L.c[p0][hi];
                const double d2 = dr * dr + dc * dc;
                q = quantise(p.wm * (d2 < p.tt ? d2 : p.tt) / p.tt);
            }
        }
        L.d[f][threadIdx.x] = (int)q;
    }
    __syncthreads();
}

// MATRIX: the transfer matrix of the block, every lane.  Else the forward pass from `vin`, lanes 0 .. 15 (row s = 0 of the matrix holds
// the vector), with the back-pointers and the exit -> entry map.
template <bool MATRIX>
__global__ __launch_bounds__(THREADS) void track_block_kernel(Params p, long long* __restrict__ Mout, const long long* __restrict__ vin,
                                                              unsigned char* __restrict__ bp, unsigned char* __restrict__ map) {
    __shared__ Costs L;
    __shared__ long long M[2][S * S];
    __shared__ unsigned char back[CHUNK * S];
    __shared__ unsigned char entry[2][S];
    const long long blk = blockIdx.x, chain = blk / p.nb, b = blk - chain * p.nb;
    const int c = (int)(chain / p.J), j = (int)(chain - (long long)c * p.J);
    const long long t0 = b * p.B, t1 = t0 + p.B < p.T ? t0 + p.B : p.T;
    const int tid = threadIdx.x, s = tid >> 4, k = tid & 15;
    const bool works = MATRIX || s == 0;
    if (MATRIX) M[0][tid] = s == k ? 0 : INF;   // the identity of (min, +)
    else if (works) M[0][k] = vin[(size_t)blk * S + k];
    int cur = 0;
    for (long long tc = t0; tc < t1; tc += CHUNK) {
        const int nf = (int)(t1 - tc < CHUNK ? t1 - tc : CHUNK);
        chunk_costs(p, c, j, t0, tc, nf, L);
        for (int f = 0; f < nf; ++f) {
            if (works) {
                const long long* row = &M[cur][s * S];
                const int* col = &L.d[f][k];
                long long best = sat_add(row[0], col[0]);
                int arg = 0;
#pragma unroll
                for (int kp = 1; kp < S; ++kp) {   // strictly smaller: the lowest minimising predecessor
                    const long long cand = sat_add(row[kp], col[kp * S]);
                    if (cand < best) best = cand, arg = kp;
                }
                M[cur ^ 1][tid] = sat_add(L.u[(tc - t0 + f + 1) & (RING - 1)][k], best);
                if (!MATRIX) {
                    back[f * S + k] = (unsigned char)arg;
                    entry[cur ^ 1][k] = tc + f == t0 ? (unsigned char)arg : entry[cur][arg];
                }
            }
            cur ^= 1;
            __syncthreads();
        }
        if (!MATRIX && tid < nf * S) bp[((size_t)chain * p.T + tc) * S + tid] = back[tid];
    }
    if (MATRIX) Mout[(size_t)blk * (S * S) + tid] = M[cur][tid];
    else if (works) map[(size_t)blk * S + k] = entry[cur][k];
}

__global__ __launch_bounds__(THREADS) void track_carry_kernel(const long long* __restrict__ M, long long nchain, long long nb,
                                                              long long* __restrict__ vin, long long* __restrict__ cost, int* __restrict__ last) {
    const long long chain = (long long)blockIdx.x * (THREADS / S) + (threadIdx.x >> 4);
    const int k = threadIdx.x & 15;
    const bool on = chain < nchain;
    long long v = k == 0 ? 0 : INF;
    for (long long b = 0; b < nb; ++b) {
        const size_t blk = on ? (size_t)chain * nb + b : 0;
        if (on) vin[blk * S + k] = v;
        long long best = INF;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const long long vs = __shfl(v, s, S);
            const long long cand = sat_add(vs, on ? M[blk * (S * S) + s * S + k] : 0);
            best = cand < best ? cand : best;
        }
        v = best;
    }
    long long mn = v;
#pragma unroll
    for (int o = S / 2; o > 0; o >>= 1) {
        const long long other = __shfl_xor(mn, o, S);
        mn = other < mn ? other : mn;
    }
    const unsigned row = (unsigned)(__ballot(v == mn) >> (threadIdx.x & 48)) & 0xffffu;
    if (on && k == 0) {
        cost[chain] = mn;
        last[chain] = __ffs(row) - 1;   // the lowest slot among the minima
    }
}

__global__ __launch_bounds__(THREADS) void track_exit_kernel(const unsigned char* __restrict__ map, const int* __restrict__ last, long long nchain,
                                                             long long nb, unsigned char* __restrict__ exit) {
    const long long chain = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (chain >= nchain) return;
    int k = last[chain];
    for (long long b = nb - 1; b >= 0; --b) {
        const size_t blk = (size_t)chain * nb + b;
        exit[blk] = (unsigned char)k;
        k = map[blk * S + k];
    }
}

__global__ __launch_bounds__(THREADS) void track_trace_kernel(const unsigned char* __restrict__ bp, const unsigned char* __restrict__ exit, long long T,
                                                              int J, long long B, long long nb, int* __restrict__ choice) {
    __shared__ uint4 table[TRACE];   // 16 back-pointers per frame
    __shared__ int chosen[TRACE];
    const long long blk = blockIdx.x, chain = blk / nb, b = blk - chain * nb;
    const int c = (int)(chain / J), j = (int)(chain - (long long)c * J);
    const long long t0 = b * B, t1 = t0 + B < T ? t0 + B : T;
    const int tid = threadIdx.x;
    int k = exit[blk];
    for (long long hi = t1; hi > t0; hi -= TRACE) {
        const long long lo = hi - TRACE > t0 ? hi - TRACE : t0;
        const int n = (int)(hi - lo);
        if (tid < n) table[tid] = reinterpret_cast<const uint4*>(bp)[(size_t)chain * T + lo + tid];
        __syncthreads();
        if (tid == 0) {
            const unsigned char* tb = reinterpret_cast<const unsigned char*>(table);
            for (int f = n - 1; f >= 0; --f) {
                chosen[f] = k;
                k = tb[f * S + k];
            }
        }
        __syncthreads();
        if (tid < n) choice[((size_t)c * T + lo + tid) * J + j] = chosen[tid];
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
long long round64(long long b) { return (b + 63) / 64 * 64; }

struct Layout {
    long long M, vin, bp, map, exit, last, bytes, nb;
};

bool sizes_ok(long long nchain, long long T, int K, int block_frames) {
    return nchain >= 1 && nchain <= CHAINS_MAX && T >= 0 && T <= 0x7fffffffLL && nchain * T <= CHAIN_FRAMES_MAX && K >= 1 && K <= K_MAX &&
           block_frames >= 1 && block_frames <= BLOCK_MAX;
}

Layout layout_of(long long nchain, long long T, int block_frames) {
    Layout l;
    l.nb = (T + block_frames - 1) / block_frames;
    const long long blocks = nchain * l.nb;
    l.M = 0;
    l.vin = l.M + round64(blocks * S * S * 8);
    l.bp = l.vin + round64(blocks * S * 8);
    l.map = l.bp + round64(nchain * T * S);
    l.exit = l.map + round64(blocks * S);
    l.last = l.exit + round64(blocks);
    l.bytes = l.last + round64(nchain * 4);
    return l;
}

template <typename P>
P* at(void* work, long long offset) {
    return reinterpret_cast<P*>(static_cast<char*>(work) + offset);
}

}  // namespace

extern "C" long long df3d_track_work_bytes(long long nchain, long long T, int K, int block_frames) {
    return sizes_ok(nchain, T, K, block_frames) ? layout_of(nchain, T, block_frames).bytes : 0;
}

extern "C" int df3d_track_peaks(const int* count_dev, const float* pts_dev, const float* val_dev, int C, long long T, int J, int K, double height_px,
                                double width_px, double tau, double w_motion, double w_value, int block_frames, int* choice_dev,
                                long long* cost_dev, void* work_dev, long long work_len_bytes, void* stream) {
    DF3D_CHECK_ARG(C >= 1 && J >= 1 && (long long)C * J <= CHAINS_MAX, "C and J must be >= 1 and C J at most 2^20");
    DF3D_CHECK_ARG(T >= 0 && T <= 0x7fffffffLL && (long long)C * J * T <= CHAIN_FRAMES_MAX, "T must be in [0, 2^31 - 1] and C J T at most 2^36");
    DF3D_CHECK_ARG(K >= 1 && K <= K_MAX, "K must be in [1, 16]");
    DF3D_CHECK_ARG(std::isfinite(height_px) && height_px > 0.0 && std::isfinite(width_px) && width_px > 0.0,
                   "height_px and width_px must be finite and > 0");
    DF3D_CHECK_ARG(std::isfinite(tau) && tau > 0.0, "tau must be finite and > 0");
    DF3D_CHECK_ARG(std::isfinite(w_motion) && w_motion >= 0.0 && w_motion <= W_MAX, "w_motion must be finite and in [0, 1024]");
    DF3D_CHECK_ARG(std::isfinite(w_value) && w_value >= 0.0 && w_value <= W_MAX, "w_value must be finite and in [0, 1024]");
    DF3D_CHECK_ARG(block_frames >= 1 && block_frames <= BLOCK_MAX, "block_frames must be in [1, 4096]");
    DF3D_CHECK_ARG((double)T * (w_motion + w_value) * SCALE < 0x1p60, "T (w_motion + w_value) 2^20 must be below 2^60");
    if (T == 0) return DF3D_OK;
    const long long nchain = (long long)C * J;
    const Layout l = layout_of(nchain, T, block_frames);
    DF3D_CHECK_ARG(nchain * l.nb <= 0x7fffffffLL, "C J ceil(T / block_frames) must be at most 2^31 - 1: use larger blocks");
    DF3D_CHECK_ARG(work_len_bytes >= l.bytes, "work buffer too small (df3d_track_work_bytes)");
    DF3D_BUFFERS({"count", count_dev, nchain * T * 4, 4}, {"pts", pts_dev, nchain * T * K * 8, 4}, {"val", val_dev, nchain * T * K * 4, 4},
                 {"choice", choice_dev, nchain * T * 4, 4}, {"cost", cost_dev, nchain * 8, 8}, {"work", work_dev, l.bytes, 16});
    hipStream_t st = df3d::as_stream(stream);
    const Params p = {count_dev, pts_dev, val_dev, T, block_frames, l.nb, J, K, height_px, width_px, tau * tau, w_motion, w_value};
    long long *M = at<long long>(work_dev, l.M), *vin = at<long long>(work_dev, l.vin);
    unsigned char *bp = at<unsigned char>(work_dev, l.bp), *map = at<unsigned char>(work_dev, l.map), *exit = at<unsigned char>(work_dev, l.exit);
    int* last = at<int>(work_dev, l.last);
    const dim3 block(THREADS), blocks((unsigned)(nchain * l.nb));
    hipLaunchKernelGGL(track_block_kernel<true>, blocks, block, 0, st, p, M, vin, bp, map);
    hipLaunchKernelGGL(track_carry_kernel, dim3((unsigned)((nchain + THREADS / S - 1) / (THREADS / S))), block, 0, st, M, nchain, l.nb, vin, cost_dev, last);
    hipLaunchKernelGGL(track_block_kernel<false>, blocks, block, 0, st, p, M, vin, bp, map);
    hipLaunchKernelGGL(track_exit_kernel, dim3((unsigned)((nchain + THREADS - 1) / THREADS)), block, 0, st, map, last, nchain, l.nb, exit);
    hipLaunchKernelGGL(track_trace_kernel, blocks, block, 0, st, bp, exit, T, J, (long long)block_frames, l.nb, choice_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
