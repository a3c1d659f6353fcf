// =====================================================================================================
// Fused pre-activation bottleneck  (256 -> 128 -> 128 -> 256, the block that makes up 29 of the network's
// 32 bottlenecks):    out = W3 relu(bn3(W2 (*) relu(bn2(W1 relu(bn1 x))))) + x
// One workgroup = one 8 x 16 output tile.  x is read once (10 x 18 halo tile), the output written once; the two
// 128-channel intermediates never leave the CU:
//   phase 1  t1 = relu(W1' relu(bn1 x) + b1')  on the 180 halo pixels (GEMM 192 x 128 x 256) -> LDS [180][128],
//            out-of-image halo pixels forced to 0 (= the zero padding of the 3x3 convolution).
//            Wave w owns output channels 32w..32w+31 for all 6 pixel tiles (x fragments are shared through LDS).
//   phase 2  t2^T = W2' (*) t1: rows = output channels (A = W2 taps, staged), columns = the wave's 32 pixels
//            (B = t1 read straight from the LDS tile at the tap-shifted pixel) -> 4 accumulator tiles per wave.
//   phase 3  out = W3 relu(t2 + b2') + b3 + x.  The transposed phase-2 accumulators ARE valid MFMA A operands:
//            accumulator register r of channel tile m holds, for pixel lane&31, channel 32m + (r&3) + 8(r>>2) +
//            4(lane>>5) -- a permutation of K that is matched on the W3 side by which 16-byte chunk a lane reads
//            (f32) / by the host's K order of the packed W3 (bf16).  So t2 never goes through LDS.
// LDS (fp32): t1 180 x 528 B = 95 KB + staging 51 KB (phase 1) / 37 KB (phases 2, 3) -> one workgroup per CU.
// =====================================================================================================
#pragma once
#include "hg_pool.h"
#include "hg_types.h"

namespace hgk {

struct BottleneckArgs {
    const void* in;     // NHWC [V, H, W, CIN]
    const void* in2;    // UP: NHWC [V, H/2, W/2, CIN]; the block's input is in + nearest-upsample(in2), rounded to T
    const void* add2;   // ADD2: NHWC [V, H/2, W/2, 2*PL]; the block WRITES out + nearest-upsample(add2) (the hourglass' up-path sum,
                        // what upadd_kernel would have made of `out`: same roundings, in the same order)
    void* out;          // NHWC [V, H, W, 2*PL]
    void* pool;         // optional NHWC [V, H/2, W/2, 2*PL]: 2x2 max-pool of `out`, written by the same epilogue
    const void* w1;     // [PL][CIN]
    const void* w2;     // [9][PL][PL]
    const void* w3;     // [2*PL][PL]      (K permuted for bf16)
    const void* wd;     // [2*PL][CIN]     downsample (skip) convolution, DS only
    const float* b1;    // [PL]   (bn2 folded)
    const float* b2;    // [PL]   (bn3 folded)
    const float* b3;    // [2*PL] (DS: conv3 bias + downsample bias, summed by the engine at set_weights time)
    const float* bd;    // [2*PL] DS only
    const float* s1;    // [CIN] bn1 scale
    const float* t1;    // [CIN] bn1 shift
    int V, H, W;
};

constexpr int BT_TH = 8, BT_TW = 16;              // output tile
constexpr int BT_HW = BT_TW + 2;                  // halo tile width (18)
constexpr int BT_HALO = (BT_TH + 2) * BT_HW;      // 180 halo pixels
constexpr int BT_HROWS = 192;                     // padded to 6 MFMA row tiles

// CIN -> PL -> PL -> 2*PL; DS: the skip path is a 1x1 convolution of the raw input (CIN != 2*PL)
template <typename T, int CIN, int PL, bool DS>
struct BtCfg {
    static constexpr int EB = Elem<T>::BYTES;
    static constexpr int CO = 2 * PL;
    // fp32, PL = 128: the t1 tile is built and consumed in TWO halves of 64 channels (phase 1 twice over x, phase 2
    // accumulates tap x channel-half), which halves its LDS footprint; with a single staging buffer the workgroup
    // then needs 73 KB instead of 153 KB and two workgroups share a CU, as in bf16.
    static constexpr int KSPLIT = (EB == 4 && PL == 128) ? 2 : 1;
    static constexpr int T1W = PL / KSPLIT;                        // channels of t1 resident at a time
    static constexpr int T1_PITCH = T1W * EB + 16;                 // bytes per halo pixel in the t1 tile
    static constexpr int T1_BYTES = BT_HROWS * T1_PITCH;           // 192 rows: the 12 pad rows make the phase-1 epilogue branch-free
    static constexpr int RB1 = 64;                                 // staged row bytes, phase 1
    static constexpr int RB2 = 128;                                // phases 2 and 3 (K = PL)
    // ONE staging buffer (two barriers per K-step) so that the workgroup needs < 80 KB of LDS and two workgroups
    // share a CU -- the second one's MFMAs cover the first one's barrier / LDS / memory stalls.
    static constexpr int RBD = 64;                                 // downsample steps of phase 3 (K = CIN)
    static constexpr int STAGE1 = (BT_HROWS + T1W) * (RB1 + 16);   // x rows + W1 rows
    static constexpr int STAGE2 = 128 * (RB2 + 16);                // W2 (PL rows) / W3 (128 rows) 
    static constexpr int STAGED = DS ? (128 + 128) * (RBD + 16) : 0;  // x centre rows + Wd rows
    static constexpr int SMAX = STAGE1 > STAGE2 ? (STAGE1 > STAGED ? STAGE1 : STAGED) : (STAGE2 > STAGED ? STAGE2 : STAGED);
    static constexpr int STAGE_BYTES = SMAX;
    static constexpr int MISC = 64;                                // halo validity masks (3 x 64 bit)
    static constexpr int LDS_BYTES = T1_BYTES + STAGE_BYTES + MISC;
    static constexpr int NT = PL / 32;                             // channel tiles of the intermediates
};

template <typename T, int CIN, int PL, bool DS, bool UP = false, bool ADD2 = false>
__global__ __launch_bounds__(256, 2) void bottleneck_kernel(BottleneckArgs p) {
    using C = BtCfg<T, CIN, PL, DS>;
    static_assert(!UP || !DS, "the upsample-add input exists for the identity-skip block only");
    static_assert(!ADD2 || (!DS && !UP), "the fused up-path sum is written by plain identity-skip blocks");
    constexpr int EB = C::EB;
    constexpr int CO = C::CO;
    constexpr int NT = C::NT;
    constexpr int PER16 = Elem<T>::PER16;
    static_assert(PL == 128 || PL == 64, "planes");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const t1_lds = smem;
    unsigned char* const stage = smem + C::T1_BYTES;
    unsigned long long* const valid_lds = reinterpret_cast<unsigned long long*>(smem + C::T1_BYTES + C::STAGE_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5;          // which 16-byte chunk of a 32-byte K group this lane reads
    const int l31 = lane & 31;
    const int tiles_x = p.W / BT_TW, tiles_y = p.H / BT_TH;
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * BT_TW;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * BT_TH;
    const int view = b / tiles_y;
    const unsigned char* const xin = reinterpret_cast<const unsigned char*>(p.in) + (size_t)view * p.H * p.W * CIN * EB;
    // UP: the low-resolution addend (the hourglass' up-path: x = in + upsample(in2), what upadd_kernel would have written)
    const unsigned char* const xin2 = UP ? reinterpret_cast<const unsigned char*>(p.in2) + (size_t)view * (p.H / 2) * (p.W / 2) * CIN * EB : nullptr;
    const unsigned char* const lo2 = ADD2 ? reinterpret_cast<const unsigned char*>(p.add2) + (size_t)view * (p.H / 2) * (p.W / 2) * CO * EB : nullptr;

    // validity of the 192 halo rows (inside the image?) as three 64-bit masks
    if (tid < BT_HROWS) {
        const int hy = tid / BT_HW, hx = tid % BT_HW;
        const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
        const bool ok = tid < BT_HALO && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) valid_lds[wave] = m;
    }

    // =========================== phase 2: t2^T = W2' (*) t1 ==============================================
    // (declarations first: phase 1 and phase 2 alternate when the t1 tile is built in channel parts)
    constexpr int RB = C::RB2, PITCH = RB + 16, CPR = RB / 16, RPP = 256 / CPR;
    constexpr int KE = RB / EB;
    const int chunk = tid % CPR, srow = tid / CPR;
    constexpr int WPASS = 128 / RPP;   // passes for 128 rows (W3 half); W2 has PL rows
    u32x4 rw[WPASS];
    auto load_w = [&](const void* wbase, int rows, size_t row_stride_elems, size_t elem_off) {
#pragma unroll
        for (int i = 0; i < WPASS; ++i)
            if (PL == 128 || srow + i * RPP < rows)  // compile-time true for PL = 128 (all tiles have 128 rows)
                rw[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(wbase) +
                                                        ((size_t)(srow + i * RPP) * row_stride_elems + elem_off + chunk * PER16) * EB);
    };
    auto store_w = [&](int buf, int rows) {
        unsigned char* const sw = stage + buf * C::SMAX;
#pragma unroll
        for (int i = 0; i < WPASS; ++i)
            if (PL == 128 || srow + i * RPP < rows) *reinterpret_cast<u32x4*>(sw + (srow + i * RPP) * PITCH + chunk * 16) = rw[i];
    };

    // this wave's 32 pixels: tile rows 2*wave, 2*wave + 1
    const int py = 2 * wave + (l31 >> 4), px = l31 & 15;
    // =========================== phase 1: t1 = relu(W1' relu(bn1 x) + b1') on the halo ===================
    // (kh: which T1W-channel part of t1 is produced: rows kh*T1W.. of W1)
    auto phase1 = [&](int kh) {
        constexpr int RB = C::RB1, PITCH = RB + 16, CPR = RB / 16, RPP = 256 / CPR;   // 4 chunks/row, 64 rows/pass
        constexpr int KE = RB / EB;
        constexpr int T1W = C::T1W, NT1 = T1W / 32;
        constexpr int XP = BT_HROWS / RPP, WP = T1W / RPP;                             // 3 and 2 (1) passes
        constexpr int X_BYTES = BT_HROWS * PITCH;
        constexpr int NSTEPS = CIN / KE;
        // wave -> (channel tile ct, row tiles rt0 .. rt0 + RT - 1)
        constexpr int RT = 6 * NT1 / 4;
        const int ct = wave % NT1, rt0 = (wave / NT1) * RT;
        const int chunk = tid % CPR, srow = tid / CPR;
        const unsigned char* xp[XP];
        const unsigned char* xq[UP ? XP : 1];
        bool xok[XP];
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const int hp = srow + i * RPP;
            const int hy = hp / BT_HW, hx = hp % BT_HW;
            const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
            xok[i] = hp < BT_HALO && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
            xp[i] = xin + ((size_t)(xok[i] ? y : 0) * p.W + (xok[i] ? x : 0)) * CIN * EB;
            if constexpr (UP) xq[i] = xin2 + ((size_t)(xok[i] ? (y >> 1) : 0) * (p.W / 2) + (xok[i] ? (x >> 1) : 0)) * CIN * EB;
        }
        u32x4 rx[XP], rw[WP];
        u32x4 rb[(UP && EB == 2) ? XP : 1];
        int c0_late = 0;
        PreactCoef<T> coef;
        auto load1 = [&](int s) {
            const int c0 = s * KE + chunk * PER16;
            coef.load(p.s1, p.t1, c0);
            // out-of-image halo rows read pixel (0,0) (a valid address) and are masked to zero in store1: no branches
#pragma unroll
            for (int i = 0; i < XP; ++i) rx[i] = *reinterpret_cast<const u32x4*>(xp[i] + (size_t)c0 * EB);
            if constexpr (UP && EB == 2) {
#pragma unroll
                for (int i = 0; i < XP; ++i) rb[i] = *reinterpret_cast<const u32x4*>(xq[i] + (size_t)c0 * EB);
            }
            if constexpr (UP && EB == 4) c0_late = c0;
#pragma unroll
            for (int i = 0; i < WP; ++i)
                rw[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(p.w1) + ((size_t)(kh * T1W + srow + i * RPP) * CIN + c0) * EB);
        };
        auto store1 = [&](int buf) {
            unsigned char* const sx = stage + buf * C::STAGE1;
            unsigned char* const sw = sx + X_BYTES;
#pragma unroll
            for (int i = 0; i < XP; ++i) {
                u32x4 v = rx[i];
                // x = in + upsample(in2), rounded like upadd_kernel's output.  bf16 prefetched the addend with x; fp32 (no
                // registers to spare beside its 254) fetches it here: a 4x re-used, L2-resident tensor
                if constexpr (UP && EB == 2) v = add_chunk<T>(v, rb[i]);
                if constexpr (UP && EB == 4) v = add_chunk<T>(v, *reinterpret_cast<const u32x4*>(xq[i] + (size_t)c0_late * EB));
                v = preact_apply<T>(v, coef);  // bn1 + ReLU, deferred past the MFMAs
                const unsigned keep = xok[i] ? 0xffffffffu : 0u;
                v &= keep;
                *reinterpret_cast<u32x4*>(sx + (srow + i * RPP) * PITCH + chunk * 16) = v;
            }
#pragma unroll
            for (int i = 0; i < WP; ++i) *reinterpret_cast<u32x4*>(sw + (srow + i * RPP) * PITCH + chunk * 16) = rw[i];
        };
        f32x16 acc[RT];
        {
            const float bias1 = p.b1[kh * T1W + ct * 32 + l31];   // bias folded into the accumulator start value
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] = bias1;
        }
        load1(0);
        store1(0);
        __syncthreads();
        for (int s = 0; s < NSTEPS; ++s) {
            const unsigned char* const sx = stage + 0 * C::STAGE1;
            const unsigned char* const sw = sx + X_BYTES;
            if (s + 1 < NSTEPS) load1(s + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < RB / 32; j += 2) {   // fragment pairs (j, j + 1): one 64-byte K step (mfma_pair)
                const u32x4 w0 = *reinterpret_cast<const u32x4*>(sw + (ct * 32 + l31) * PITCH + j * 32 + half * 16);
                const u32x4 w1 = *reinterpret_cast<const u32x4*>(sw + (ct * 32 + l31) * PITCH + (j + 1) * 32 + half * 16);
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    const unsigned char* const xrow = sx + ((rt0 + i) * 32 + l31) * PITCH + half * 16;
                    mfma_pair<T, false>(w0, w1, make_xpair<T>(*reinterpret_cast<const u32x4*>(xrow + j * 32), *reinterpret_cast<const u32x4*>(xrow + (j + 1) * 32)), acc[i]);
                }
            }
            if (s + 1 < NSTEPS) __syncthreads();  // every wave is done reading the only buffer
            if (s + 1 < NSTEPS) store1(0);
            __syncthreads();
        }
        // epilogue: bias + ReLU, zero outside the image, into the t1 tile (rows = halo pixels, PL channels).
        // Branch-free: every row (also the 12 pad rows, whose validity bit is 0) is written.
        const int n = ct * 32 + l31;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const unsigned vmh = (unsigned)(valid_lds[(rt0 + i) >> 1] >> (((rt0 + i) & 1) * 32 + 4 * half));
            unsigned char* const trow = t1_lds + ((rt0 + i) * 32 + 4 * half) * C::T1_PITCH + n * EB;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                // select by bit mask (a ?: here makes hipcc emit one branch per register)
                const unsigned keep = 0u - ((vmh >> ro) & 1u);
                const float v = __uint_as_float(__float_as_uint(fmaxf(acc[i][r], 0.0f)) & keep);
                if constexpr (EB == 4)
                    *reinterpret_cast<float*>(trow + ro * C::T1_PITCH) = v;
                else
                    *reinterpret_cast<unsigned short*>(trow + ro * C::T1_PITCH) = Lp<T>::from_f32(v);
            }
        }
    };

    phase1(0);
    __syncthreads();

    // t2 accumulators start at b2' (channel of register r in tile m: 32m + (r&3) + 8(r>>2) + 4*half)
    f32x16 t2[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(p.b2 + 32 * m + 8 * q + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) t2[m][4 * q + e] = bb[e];
        }

    {
        // one staging buffer, two barriers per K-step (two workgroups per CU); kh selects the resident t1 channel part
        auto phase2 = [&](int kh) {
            constexpr int T1W = C::T1W;
            constexpr int KSTEPS = T1W / KE;         // K-steps per tap
            constexpr int NSTEPS = 9 * KSTEPS;
            load_w(p.w2, PL, PL, (size_t)kh * T1W);
            store_w(0, PL);
            __syncthreads();
            for (int s = 0; s < NSTEPS; ++s) {
                const int tap = s / KSTEPS, kc = s - tap * KSTEPS;
                const unsigned char* const sw = stage;
                if (s + 1 < NSTEPS) {
                    const int tap1 = (s + 1) / KSTEPS, kc1 = (s + 1) - tap1 * KSTEPS;
                    load_w(p.w2, PL, PL, (size_t)tap1 * PL * PL + (size_t)kh * T1W + (size_t)kc1 * KE);
                }
                __builtin_amdgcn_sched_barrier(0);
                const int ky = tap / 3, kx = tap - 3 * ky;
                const unsigned char* const tb = t1_lds + ((py + ky) * BT_HW + (px + kx)) * C::T1_PITCH + kc * RB + half * 16;
                const unsigned char* const wrow = sw + l31 * PITCH + half * 16;
                // (requesting the fragments of two K chunks before their eight MFMA groups, pinned with sched_barrier, made the fp32
                // layer1 form 2-3 % SLOWER -- at three workgroups per CU hipcc's own interleaving is the better one)
#pragma unroll
                for (int j = 0; j < RB / 32; j += 2) {   // fragment pairs (j, j + 1): one 64-byte K step (mfma_pair)
                    const XPair<T> tp = make_xpair<T>(*reinterpret_cast<const u32x4*>(tb + j * 32), *reinterpret_cast<const u32x4*>(tb + (j + 1) * 32));
#pragma unroll
                    for (int m = 0; m < NT; ++m)
                        mfma_pair<T, true>(*reinterpret_cast<const u32x4*>(wrow + m * 32 * PITCH + j * 32), *reinterpret_cast<const u32x4*>(wrow + m * 32 * PITCH + (j + 1) * 32), tp, t2[m]);
                }
                if (s + 1 < NSTEPS) __syncthreads();
                if (s + 1 < NSTEPS) store_w(0, PL);
                __syncthreads();
            }
        };
#pragma unroll 1
        for (int kh = 0; kh < C::KSPLIT; ++kh) {
            if (kh > 0) phase1(kh);
            if (kh > 0) __syncthreads();
            phase2(kh);
        }
    }

    // ReLU on t2 (the bias was the accumulator start value)
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) t2[m][r] = fmaxf(t2[m][r], 0.0f);

    // =========================== phase 3: out = W3 t2 (+ Wd x) + b + (x) ==================================
    // halves of 128 output channels; K-step = KE channels of t2 = accumulator registers of one/two tiles
#pragma unroll 1
    for (int nh = 0; nh < CO / 128; ++nh) {
        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = nh * 128 + i * 32 + l31;
            const float bias = DS ? p.b3[n] + p.bd[n] : p.b3[n];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = bias;
        }
        // identity skip, bf16: the residual values are requested NOW (their latency hides behind the K loop); fp32 at two
        // workgroups per CU has no registers to spare and loads them in the epilogue
        constexpr int NRES = (!DS && EB == 2) ? 32 : 1;
        unsigned xres[NRES];
        if constexpr (!DS) {
            if constexpr (EB == 2) {
                // bf16: the epilogue goes through LDS (see below): lane owns, for c = 0..7, the 16-byte chunk (lane & 15)
                // of wave pixel 4c + (lane >> 4) -> eight 16-byte residual loads
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int pw = 4 * c + (lane >> 4);
                    const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(xin) +
                        ((size_t)(ty0 + 2 * wave + (pw >> 4)) * p.W + (tx0 + (pw & 15))) * CIN + nh * 128 + (lane & 15) * 8);
                    xres[4 * c + 0] = v[0];
                    xres[4 * c + 1] = v[1];
                    xres[4 * c + 2] = v[2];
                    xres[4 * c + 3] = v[3];
                }
            }
        }
        constexpr int NSTEPS = PL / KE;
        const void* w3h = reinterpret_cast<const unsigned char*>(p.w3) + (size_t)nh * 128 * PL * EB;
        load_w(w3h, 128, PL, 0);
        store_w(0, 128);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            const unsigned char* const sw = stage + 0 * C::SMAX;
            if (s + 1 < NSTEPS) load_w(w3h, 128, PL, (size_t)(s + 1) * KE);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (EB == 4) {
                // one 32-channel tile per 128 staged bytes: tile index = s * (KE / 32) + mm
#pragma unroll
                for (int mm = 0; mm < KE / 32; ++mm)
#pragma unroll
                    for (int q2 = 0; q2 < 2; ++q2)
                    {
                        // registers 8*q2 + 4*jj + e hold channels 16*q2 + 8*jj + 4*half + e  -> 16-byte chunk (4*q2 + 2*jj + half): jj = 0, 1 = one K step
                        const f32x16& tt = t2[s * (KE / 32) + mm];
                        const XPair<T> tp = make_xpair<T>(tt[8 * q2], tt[8 * q2 + 1], tt[8 * q2 + 2], tt[8 * q2 + 3], tt[8 * q2 + 4], tt[8 * q2 + 5], tt[8 * q2 + 6], tt[8 * q2 + 7]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const unsigned char* const wrow3 = sw + (i * 32 + l31) * PITCH + mm * 128 + (4 * q2 + half) * 16;
                            mfma_pair<T, false>(*reinterpret_cast<const u32x4*>(wrow3), *reinterpret_cast<const u32x4*>(wrow3 + 32), tp, acc[i]);
                        }
                    }
            } else {
                // per 32-channel tile two MFMAs (registers 0-7 and 8-15).  Packed W3 K order (host): position
                // 8*(2*q + half) + e  <->  channel 16*q + 8*(e>>2) + 4*half + (e&3) within the tile
#pragma unroll
                for (int mm = 0; mm < KE / 32; ++mm)
#pragma unroll
                    for (int q2 = 0; q2 < 2; ++q2) {
                        const f32x16& tt = t2[s * (KE / 32) + mm];
                        const u32x4 af = lp_pack8<T>(tt[8 * q2], tt[8 * q2 + 1], tt[8 * q2 + 2], tt[8 * q2 + 3], tt[8 * q2 + 4], tt[8 * q2 + 5], tt[8 * q2 + 6], tt[8 * q2 + 7]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const u32x4 wf = *reinterpret_cast<const u32x4*>(sw + (i * 32 + l31) * PITCH + (mm * 32 + (2 * q2 + half) * 8) * 2);
                            acc[i] = Lp<T>::mfma(af, wf, acc[i]);
                        }
                    }
            }
            if (s + 1 < NSTEPS) __syncthreads();
            if (s + 1 < NSTEPS) store_w(0, 128);
            __syncthreads();
        }
        if constexpr (DS) {
            // skip path: acc += x_centre[32 px][CIN] * Wd[nh half][CIN]^T, both operands staged (standard orientation)
            constexpr int RBd = C::RBD, PITCHd = RBd + 16, CPRd = RBd / 16, RPPd = 256 / CPRd;   // 4 chunks/row, 64 rows/pass
            constexpr int KEd = RBd / EB, NSTEPSd = CIN / KEd;
            constexpr int XBYTES = 128 * PITCHd;
            const int chunkd = tid % CPRd, srowd = tid / CPRd;
            u32x4 rxd[2], rwd[2];
            auto loadd = [&](int s) {
                const int c0 = s * KEd + chunkd * PER16;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int pr = srowd + i * RPPd;   // pixel row 0..127 of the 8 x 16 tile
                    rxd[i] = *reinterpret_cast<const u32x4*>(xin + (((size_t)(ty0 + (pr >> 4)) * p.W + (tx0 + (pr & 15))) * CIN + c0) * EB);
                    rwd[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(p.wd) + ((size_t)(nh * 128 + pr) * CIN + c0) * EB);
                }
            };
            auto stored = [&](int buf) {
                unsigned char* const sx = stage + buf * C::SMAX;
                unsigned char* const sw = sx + XBYTES;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    *reinterpret_cast<u32x4*>(sx + (srowd + i * RPPd) * PITCHd + chunkd * 16) = rxd[i];
                    *reinterpret_cast<u32x4*>(sw + (srowd + i * RPPd) * PITCHd + chunkd * 16) = rwd[i];
                }
            };
            loadd(0);
            stored(0);
            __syncthreads();
            for (int s = 0; s < NSTEPSd; ++s) {
                const unsigned char* const sx = stage + 0 * C::SMAX;
                const unsigned char* const sw = sx + XBYTES;
                if (s + 1 < NSTEPSd) loadd(s + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < RBd / 32; j += 2) {   // fragment pairs (j, j + 1): one 64-byte K step (mfma_pair)
                    const unsigned char* const xrow = sx + (wave * 32 + l31) * PITCHd + half * 16;
                    const XPair<T> xp2 = make_xpair<T>(*reinterpret_cast<const u32x4*>(xrow + j * 32), *reinterpret_cast<const u32x4*>(xrow + (j + 1) * 32));
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned char* const wrowd = sw + (i * 32 + l31) * PITCHd + half * 16;
                        mfma_pair<T, false>(*reinterpret_cast<const u32x4*>(wrowd + j * 32), *reinterpret_cast<const u32x4*>(wrowd + (j + 1) * 32), xp2, acc[i]);
                    }
                }
                if (s + 1 < NSTEPSd) __syncthreads();
                if (s + 1 < NSTEPSd) stored(0);
                __syncthreads();
            }
        }
        // epilogue: D[row = pixel (r&3) + 8(r>>2) + 4*half of the wave][col = channel nh*128 + 32 i + l31]
        unsigned char* const outp = reinterpret_cast<unsigned char*>(p.out) + (size_t)view * p.H * p.W * CO * EB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = nh * 128 + i * 32 + l31;
            if constexpr (EB == 4) {
                if constexpr (!DS) {   // all 16 residual loads of the tile before the first store
                    float xr[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int pl = (r & 3) + 8 * (r >> 2) + 4 * half;
                        xr[r] = reinterpret_cast<const float*>(xin)[((size_t)(ty0 + 2 * wave + (pl >> 4)) * p.W + (tx0 + (pl & 15))) * CIN + n];
                    }
                    if constexpr (UP) {
                        // the wave's two tile rows share ONE half-resolution row and neighbouring columns one pixel: registers
                        // r, r^1, r^8, r^9 take the same addend -> 4 loads per tile, key = bits 1 and 2 of r
                        float t4[4];
#pragma unroll
                        for (int key = 0; key < 4; ++key)
                            t4[key] = reinterpret_cast<const float*>(xin2)[((size_t)(ty0 / 2 + wave) * (p.W / 2) + tx0 / 2 + (key & 1) + 4 * (key >> 1) + 2 * half) * CIN + n];
#pragma unroll
                        for (int r = 0; r < 16; ++r) xr[r] += t4[((r >> 1) & 1) + 2 * ((r >> 2) & 1)];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][r] += xr[r];
                }
                if constexpr (ADD2) {   // + nearest-upsample(add2): a second fp32 add, as upadd_kernel would have done on the stored tensor
                    float t4[4];
#pragma unroll
                    for (int key = 0; key < 4; ++key)
                        t4[key] = reinterpret_cast<const float*>(lo2)[((size_t)(ty0 / 2 + wave) * (p.W / 2) + tx0 / 2 + (key & 1) + 4 * (key >> 1) + 2 * half) * CO + n];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][r] += t4[((r >> 1) & 1) + 2 * ((r >> 2) & 1)];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pl = (r & 3) + 8 * (r >> 2) + 4 * half;
                    const size_t po = ((size_t)(ty0 + 2 * wave + (pl >> 4)) * p.W + (tx0 + (pl & 15))) * CO + n;
                    reinterpret_cast<float*>(outp)[po] = acc[i][r];
                }
                if (p.pool) {
                    // 2x2 max-pool inside the lane: horizontal neighbour = register r^1, vertical neighbour = r^8
                    float* const pp = reinterpret_cast<float*>(p.pool) + (size_t)view * (p.H / 2) * (p.W / 2) * CO;
#pragma unroll
                    for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
                        for (int b2 = 0; b2 < 2; ++b2) {
                            const int r0 = 2 * a2 + 4 * b2;
                            const float v = fmaxf(fmaxf(acc[i][r0], acc[i][r0 + 1]), fmaxf(acc[i][r0 + 8], acc[i][r0 + 9]));
                            const int ppx = a2 + 4 * b2 + 2 * half;
                            pp[((size_t)(ty0 / 2 + wave) * (p.W / 2) + (tx0 / 2 + ppx)) * CO + n] = v;
                        }
                }
            }
        }
        if constexpr (EB == 2) {
            // bf16 epilogue through LDS: 4-byte-per-lane global stores cost 17 % of the kernel; instead every wave
            // parks its 32 px x 128 ch tile (bf16) in its own slice of the dead t1 region and streams it out as
            // 16-byte chunks: per lane 8 x (ds_read_b128 + residual add + global_store_dwordx4), rows fully coalesced.
            // Only this wave touches its slice, so no barrier is needed (LDS operations of a wave complete in order).
            constexpr int OP = 128 * 2 + 16;                    // slice row pitch (bytes)
            unsigned char* const slice = t1_lds + wave * (32 * OP);
            const int odd = lane & 1;
            u32x4 x2[(UP || ADD2) ? 4 : 1];
            if constexpr (UP || ADD2) {  // low-resolution addend (UP: of the residual; ADD2: of the output): pixel (row wave of the
                                         // half-size tile, column pw/2); chunks c and c + 4 (the tile row below) share it
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int pw = 4 * c + (lane >> 4);
                    x2[c] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(UP ? xin2 : lo2) +
                        ((size_t)(ty0 / 2 + wave) * (p.W / 2) + ((tx0 + (pw & 15)) >> 1)) * CIN + nh * 128 + (lane & 15) * 8);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int rr = 2 * q + odd;                 // lane pairs exchange one register: see the stem epilogue
                    const int pl = (rr & 3) + 8 * (rr >> 2) + 4 * half;
                    const float va = acc[i][2 * q], vb = acc[i][2 * q + 1];
                    const float g = __shfl_xor(odd ? va : vb, 1, 64);
                    *reinterpret_cast<unsigned*>(slice + pl * OP + (i * 32 + (l31 & ~1)) * 2) = Lp<T>::pack2(odd ? g : va, odd ? vb : g);
                }
            unsigned short* const outs = reinterpret_cast<unsigned short*>(outp);
            u32x4 fin[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int pw = 4 * c + (lane >> 4);
                u32x4 v = *reinterpret_cast<const u32x4*>(slice + pw * OP + (lane & 15) * 16);
                if constexpr (!DS) {
                    u32x4 x4 = {xres[4 * c], xres[4 * c + 1], xres[4 * c + 2], xres[4 * c + 3]};
                    if constexpr (UP) x4 = add_chunk<T>(x4, x2[c & 3]);
                    v = add_chunk<T>(v, x4);
                }
                if constexpr (ADD2) v = add_chunk<T>(v, x2[c & 3]);   // the rounded block output + the low-resolution tensor, rounded again
                fin[c] = v;
                *reinterpret_cast<u32x4*>(outs + ((size_t)(ty0 + 2 * wave + (pw >> 4)) * p.W + (tx0 + (pw & 15))) * CO + nh * 128 + (lane & 15) * 8) = v;
            }
            if (p.pool) {
                // pooled tile row `wave`: horizontal neighbour = lane ^ 16 (pixel +-1), vertical neighbour = chunk c + 4
                unsigned short* const pp = reinterpret_cast<unsigned short*>(p.pool) + (size_t)view * (p.H / 2) * (p.W / 2) * CO;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    u32x4 m = max_chunk<T>(fin[c], fin[c + 4]);
                    u32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = __shfl_xor(m[e], 16, 64);
                    m = max_chunk<T>(m, o);
                    if (((lane >> 4) & 1) == 0)
                        *reinterpret_cast<u32x4*>(pp + ((size_t)(ty0 / 2 + wave) * (p.W / 2) + (tx0 / 2 + 2 * c + (lane >> 5))) * CO + nh * 128 + (lane & 15) * 8) = m;
                }
            }
        }
    }
}

}  // namespace hgk
