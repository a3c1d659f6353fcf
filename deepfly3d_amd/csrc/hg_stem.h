// The hourglass stem: 7x7 / stride 2 / pad 3 convolution 3 -> 64 with folded BN + ReLU.  images f32 NHWC [V, H, W, 3], or camera frames
// sampled on the fly (StemU8).  One workgroup = 8 x 16 output pixels x 64 channels; the 21 x 37 x 3 input patch and the whole weight
// matrix live in LDS.  Three kernels, one per operand format, share everything but their K loops:
//   stem_kernel<T>      exact fp32: K index k = ky*21 + kx*3 + c (a patch row is contiguous in k), v_mfma_f32_32x32x2_f32
//   stem_lp_kernel<T>   16-bit engines: K ky-major with 24 slots per patch row, 11 steps of v_mfma_f32_32x32x16_bf16 / _f16
//   stem_f32s_kernel    stem_lp_kernel's layout with both operands as IEEE-half hi / lo pairs, float32 output
// All three are PERSISTENT (stem_walk): a workgroup walks tiles b, b + gridDim.x, ...; the weights enter LDS once per workgroup and the
// next tile's patch is gathered into registers before the K loop and written to the (single) patch buffer behind it, so that no tile
// after the first waits for its input.
//
// The geometry below is the only place that states it: the plan sizes the stem's weight slot from it (hg_plan.h), the re-layout
// launches and the hi / lo offset follow from it (hg_weights.h), and so do the grids (hg_launch.h).
#pragma once
#include "hg_types.h"
#include "preprocess_math.h"

namespace hgk {

// camera frames as the stem's input (df3d_hg_forward_u8): the patch values are sampled from the uint8 frames with the front-end's
// arithmetic (preprocess_math.h) instead of being read from a float image
struct StemU8 {
    const unsigned char* frames;   // [V][FH][FW][FC] uint8, or nullptr: read StemArgs::img
    const unsigned char* flip;     // [V] or nullptr
    int FH, FW, FC;
    df3d_pre::Norm nm;
};

struct StemArgs {
    const float* img;    // [V, H, W, 3] f32 (unread when u8.frames is set)
    void* out;           // NHWC [V, H/2, W/2, 64] (T; float for stem_f32s_kernel)
    const float* w;      // stem_kernel: [148][64] f32, k-major (row 147 = 0), as it lies in the blob
    const void* w_lp;    // stem_lp_kernel: the [64][184] 16-bit tile, k' = ky*24 + kx*3 + c (stem_relayout_kernel);
                         // stem_f32s_kernel: two such IEEE-half tiles, hi then lo (stem_relayout_f32s_kernel); stem_kernel: unread
    const float* bias;   // [64]
    int V, H, W;         // input size
    StemU8 u8;
};

constexpr int STEM_TH = 8, STEM_TW = 16;                                     // output tile
constexpr int STEM_PR = 2 * STEM_TH + 5, STEM_PC = 2 * STEM_TW + 5;          // input patch: 21 rows x 37 pixels (x 3 channels)
constexpr int STEM_NIT = (STEM_PR * STEM_PC + 255) / 256;                    // patch pixels per thread (4; the last round is partial)
constexpr int STEM_KTOT = 148;                                               // fp32 weight rows: 7 * 21 taps + one of zeros
constexpr int STEM_F32_PROW = 112;                                           // fp32 patch: floats per row (111 + a zero cell)
constexpr int STEM_F32_W_BYTES = STEM_KTOT * 64 * 4;                         // 37 KB
constexpr int STEM_KP = 176, STEM_WPITCH = STEM_KP + 8;                      // 16-bit weight row: 7 * 24 = 168 k', padded to 11 MFMA steps, + 8 (368 B:
                                                                             // conflict-free 16-byte reads)
constexpr int STEM_LP_PROW = 120;                                            // 16-bit patch: elements per row (111 used; 240 B, a multiple of 16)
constexpr int STEM_LP_PATCH_ELEMS = STEM_PR * STEM_LP_PROW + 64;             // ... and 64 behind the last row, read by the last K slots
constexpr int STEM_LP_TILE_ELEMS = 64 * STEM_WPITCH;                         // the [64][184] tile: what the stem's weight slot is sized for
constexpr int STEM_LP_TILE_BYTES = STEM_LP_TILE_ELEMS * 2;                   // 23 552: where the f32s lo tile starts
constexpr int STEM_F32S_W_BYTES = 2 * STEM_LP_TILE_BYTES;                    // 47 104 = the slot in the float32-sized pre-split copy, exactly
static_assert(STEM_PR == 21 && STEM_PC == 37 && STEM_NIT == 4, "stem patch");
static_assert(STEM_F32_W_BYTES % 1024 == 0 && STEM_LP_TILE_BYTES % 1024 == 0, "the weights are copied in whole 1 KB pieces");
static_assert(STEM_F32S_W_BYTES == STEM_LP_TILE_ELEMS * 4, "the hi / lo tiles fill the float32 slot");
// workgroups per CU of the persistent grids (hg_launch.h), by the LDS a workgroup takes of the CU's 160 KB
constexpr int STEM_F32_WGS_PER_CU = 3;    // 47 KB (with two patch buffers, two workgroups: 8 % slower)
constexpr int STEM_LP_WGS_PER_CU = 4;     // 29 KB
constexpr int STEM_F32S_WGS_PER_CU = 2;   // 57 KB

struct StemTile {
    int view, ty0, tx0;   // view, first output row and column
};
struct StemGrid {
    int OH, OW, tiles_x, tiles_y, ntiles;
    __device__ __forceinline__ explicit StemGrid(const StemArgs& p)
        : OH(p.H / 2), OW(p.W / 2), tiles_x(OW / STEM_TW), tiles_y(OH / STEM_TH), ntiles(p.V * tiles_y * tiles_x) {}
    __device__ __forceinline__ StemTile tile(int b) const {
        const int tx0 = (b % tiles_x) * STEM_TW;
        b /= tiles_x;
        const int ty0 = (b % tiles_y) * STEM_TH;
        return StemTile{b / tiles_y, ty0, tx0};
    }
};

// the weights as they lie in global memory -> LDS: PIECES one-KB pieces by LDS-DMA, wave w taking pieces w, w + 4, ... (no registers, no
// ds_write; runs under the patch staging).  A wave's pieces have landed after its s_waitcnt vmcnt(0).
template <int PIECES>
__device__ __forceinline__ void stem_copy_weights(const void* src, void* lds, int tid) {
    const unsigned dst = lds_addr(lds);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int k = 0; k < (PIECES + 3) / 4; ++k) {
        const int pc = wv + 4 * k;
        if (pc < PIECES) br_glds_piece(src, (unsigned)pc * 1024u + (unsigned)(tid & 63) * 16u, dst + (unsigned)pc * 1024u);
    }
}

// This thread's share of tile t's input patch -> registers.  One item = one patch pixel (three contiguous floats): index arithmetic and
// bounds test per pixel, not per value; ALL of a thread's items are requested before the first is stored.  The engine's only call of
// df3d_pre::pixel: what makes df3d_hg_forward_u8 bit-identical to preprocess + forward.
__device__ __forceinline__ void stem_gather(const StemArgs& p, const StemGrid& g, int t, int tid, float (&pv)[STEM_NIT][3]) {
    const StemTile tl = g.tile(t);
    const int iy0 = 2 * tl.ty0 - 3, ix0 = 2 * tl.tx0 - 3;
    const float* img = p.img + (size_t)tl.view * p.H * p.W * 3;
#pragma unroll
    for (int j = 0; j < STEM_NIT; ++j) {
        const int i = tid + 256 * j;
        const int r = i / STEM_PC, pxl = i - r * STEM_PC;
        const int y = iy0 + r, x = ix0 + pxl;
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (i < STEM_PR * STEM_PC && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W) {
            if (p.u8.frames) {
                float res[3];
                df3d_pre::pixel(p.u8.frames + (size_t)tl.view * p.u8.FH * p.u8.FW * p.u8.FC, p.u8.FH, p.u8.FW, p.u8.FC, p.u8.flip && p.u8.flip[tl.view], p.H,
                                p.W, y, x, p.u8.nm, res);
                v0 = res[0];
                v1 = res[1];
                v2 = res[2];
            } else {
                const float* const src = img + ((size_t)y * p.W + x) * 3;
                v0 = src[0];
                v1 = src[1];
                v2 = src[2];
            }
        }
        pv[j][0] = v0;
        pv[j][1] = v1;
        pv[j][2] = v2;
    }
}

// the gathered pixels -> the LDS patch: put(patch offset of the pixel's first value in units of one value at a row pitch of PROW, its three values)
template <int PROW, typename Put>
__device__ __forceinline__ void stem_scatter(int tid, const float (&pv)[STEM_NIT][3], Put put) {
#pragma unroll
    for (int j = 0; j < STEM_NIT; ++j) {
        const int i = tid + 256 * j;
        if (i < STEM_PR * STEM_PC) {
            const int r = i / STEM_PC, pxl = i - r * STEM_PC;
            put(r * PROW + 3 * pxl, pv[j]);
        }
    }
}

// 16-bit patches: the pad cells behind the 111 values of a row and behind the last row (read by the last K slots against zero weights)
// are zero; no tile writes them.  lo: the second patch of the f32s stem.
__device__ __forceinline__ void stem_lp_zero_pads(int tid, unsigned short* patch, unsigned short* lo = nullptr) {
    constexpr int PADS = STEM_LP_PROW - STEM_PC * 3;
    for (int i = tid; i < STEM_PR * PADS + 64; i += 256) {
        const int r = i / PADS, c = i - r * PADS;
        const int at = i < STEM_PR * PADS ? r * STEM_LP_PROW + STEM_PC * 3 + c : STEM_PR * STEM_LP_PROW + (i - STEM_PR * PADS);
        patch[at] = 0;
        if (lo) lo[at] = 0;
    }
}

// The persistent tile walk.  tile_body(tile) is the K loop and the epilogue of one tile, reading the LDS patch; scatter() writes the
// registers that stem_gather filled to that patch.
template <typename Scatter, typename TileBody>
__device__ __forceinline__ void stem_walk(const StemArgs& p, const StemGrid& g, int tid, float (&pv)[STEM_NIT][3], Scatter scatter, TileBody tile_body) {
    int tile = blockIdx.x;
    for (;;) {
        const int next = tile + (int)gridDim.x;
        const bool has_next = next < g.ntiles;
        if (has_next) stem_gather(p, g, next, tid, pv);   // requested now, consumed behind the K loop
        tile_body(tile);
        if (!has_next) break;
        __syncthreads();   // every wave is done reading the patch
        scatter();
        __syncthreads();
        tile = next;
    }
}

// Epilogue with lane = channel, register = pixel (the C layout of the 32x32 MFMA): bias + ReLU, 128 (fp32) contiguous bytes per pixel and
// channel half.  stem_kernel<T> and, with T = float, stem_f32s_kernel.
template <typename T>
__device__ __forceinline__ void stem_store(const StemArgs& p, const StemGrid& g, int tile, int lane, int wave, const f32x16& acc0, const f32x16& acc1,
                                           float bias0, float bias1) {
    const StemTile tl = g.tile(tile);
    const int n = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mm = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int oy = tl.ty0 + wave * 2 + (mm >> 4), ox = tl.tx0 + (mm & 15);
        const size_t o = (((size_t)tl.view * g.OH + oy) * g.OW + ox) * 64;
        const float v0 = fmaxf(acc0[r] + bias0, 0.0f), v1 = fmaxf(acc1[r] + bias1, 0.0f);
        if constexpr (sizeof(T) == 4) {
            reinterpret_cast<float*>(p.out)[o + n] = v0;
            reinterpret_cast<float*>(p.out)[o + 32 + n] = v1;
        } else {
            reinterpret_cast<unsigned short*>(p.out)[o + n] = Lp<T>::from_f32(v0);
            reinterpret_cast<unsigned short*>(p.out)[o + 32 + n] = Lp<T>::from_f32(v1);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256, 3) void stem_kernel(StemArgs p) {
    constexpr int PROW = STEM_F32_PROW, KTOT = STEM_KTOT;
    __shared__ float patch[STEM_PR * PROW];   // ONE buffer: see STEM_F32_WGS_PER_CU
    __shared__ float wl[KTOT * 64];
    const StemGrid grid(p);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= grid.ntiles) return;

    stem_copy_weights<STEM_F32_W_BYTES / 1024>(p.w, wl, tid);
    float pv[STEM_NIT][3];
    auto scatter = [&]() {
        stem_scatter<PROW>(tid, pv, [&](int at, const float (&v)[3]) {
            patch[at] = v[0];
            patch[at + 1] = v[1];
            patch[at + 2] = v[2];
        });
        if (tid < STEM_PR) patch[tid * PROW + STEM_PC * 3] = 0.0f;   // the pad cell behind the 111 values of a row
    };
    stem_gather(p, grid, blockIdx.x, tid, pv);
    scatter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's weight pieces have landed
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31;                 // pixel inside the wave's 2 x 16 sub-tile
    const int py = wave * 2 + (m >> 4), px = m & 15;
    const int a_base = (2 * py) * PROW + 6 * px;
    const int khalf = lane >> 5;
    const int n = lane & 31;
    const float bias0 = p.bias[n], bias1 = p.bias[32 + n];
    stem_walk(p, grid, tid, pv, scatter, [&](int tile) {
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
        // K step s multiplies k = 2 s (lanes 0..31) and k = 2 s + 1 (lanes 32..63); tap k lies at patch offset (k / 21) * PROW + k % 21.
        // Fully unrolled with every LDS address a register + an immediate: the offset of the ODD tap is the even one's + 1, or + PROW - 20
        // where the pair straddles two patch rows -- two base registers.  Reads run one group of four steps ahead of the MFMAs (the
        // rolled loop spent ten VALU instructions on k / 21 and waited for each step's three reads in front of its two MFMAs: 0.59
        // matrix-pipe busy).
        const float* const pa = patch + a_base + khalf;                  // odd tap = even tap + 1
        const float* const pb = patch + a_base + khalf * (PROW - 20);    // ... or first tap of the next patch row
        const float* const wb = wl + khalf * 64 + (lane & 31);
        constexpr int G = 4, NG = (KTOT / 2 + G - 1) / G;                // 74 steps in 19 groups (the last has two)
        float fa[2][G], fb0[2][G], fb1[2][G];
        auto load_group = [&](int g, int buf) {
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int s = g * G + i;
                if (s >= KTOT / 2) break;
                const int k0 = 2 * s, off0 = (k0 / 21) * PROW + k0 % 21;
                const bool straddle = k0 % 21 == 20;
                float a = straddle ? pb[off0] : pa[off0];
                if (k0 + 1 >= 147) a = khalf ? 0.0f : a;   // the 148th tap is padding
                fa[buf][i] = a;
                fb0[buf][i] = wb[k0 * 64];
                fb1[buf][i] = wb[k0 * 64 + 32];
            }
        };
        load_group(0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) load_group(g + 1, (g + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if (g * G + i >= KTOT / 2) break;
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][i], fb0[g & 1][i], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][i], fb1[g & 1][i], acc1, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        stem_store<T>(p, grid, tile, lane, wave, acc0, acc1, bias0, bias1);
    });
}

// -----------------------------------------------------------------------------------------------------
// stem for the 16-bit engines (T = __hip_bfloat16 / _Float16).  K is laid out ky-major with every ky row padded from 21 to 24 taps
// (k' = ky*24 + kx*3 + c; 7*24 = 168, padded to 176 = 11 MFMA steps), so the 8 K-slots a lane feeds to one MFMA are 8 CONSECUTIVE
// 16-bit values of one patch row (4 ds_read_b32).  The f32 image patch is converted while it is staged; the weights were laid out once
// by stem_relayout_kernel (wl[n][ky*24 + kk] = w[ky*21 + kk][n]) from the same f32 blob the f32 stem uses.  22 MFMAs per wave instead
// of 148: the kernel becomes load/store-bound.
// -----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void stem_lp_kernel(StemArgs p) {
    constexpr int PROW = STEM_LP_PROW, KP = STEM_KP, WPITCH = STEM_WPITCH;
    __shared__ __attribute__((aligned(16))) unsigned short patch[STEM_LP_PATCH_ELEMS];
    __shared__ __attribute__((aligned(16))) unsigned short wl[STEM_LP_TILE_ELEMS];
    const StemGrid grid(p);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= grid.ntiles) return;

    stem_copy_weights<STEM_LP_TILE_BYTES / 1024>(p.w_lp, wl, tid);
    float pv[STEM_NIT][3];
    auto scatter = [&]() {
        stem_scatter<PROW>(tid, pv, [&](int at, const float (&v)[3]) {
            patch[at] = Lp<T>::from_f32(v[0]);
            patch[at + 1] = Lp<T>::from_f32(v[1]);
            patch[at + 2] = Lp<T>::from_f32(v[2]);
        });
    };
    stem_gather(p, grid, blockIdx.x, tid, pv);
    scatter();
    stem_lp_zero_pads(tid, patch);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's weight pieces have landed
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, half = lane >> 5;
    const int py = wave * 2 + (m >> 4), px = m & 15;
    const unsigned short* const abase = patch + (2 * py) * PROW + 6 * px;   // 12*px bytes: 4-byte aligned
    const unsigned short* const wrow0 = wl + m * WPITCH;
    const unsigned short* const wrow1 = wl + (32 + m) * WPITCH;
    const int n = lane & 31;
    const int odd = lane & 1;
    const float bias0 = p.bias[n], bias1 = p.bias[32 + n];
    stem_walk(p, grid, tid, pv, scatter, [&](int tile) {
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KP / 16; ++s) {
            const int kp = 16 * s + 8 * half;          // first k' of this lane's 8 slots
            const int ky = kp / 24, kk = kp % 24;       // 8 consecutive taps of patch row 2*py + ky (kk in {0, 8, 16})
            u32x4 av = {0u, 0u, 0u, 0u};
            if (kp < 168) {
                const unsigned* ap = reinterpret_cast<const unsigned*>(abase + ky * PROW + kk);
                av[0] = ap[0];
                av[1] = ap[1];
                av[2] = ap[2];
                av[3] = ap[3];   // taps 21..23 of the row multiply zero weights
            }
            const u32x4 b0 = *reinterpret_cast<const u32x4*>(wrow0 + kp);
            const u32x4 b1 = *reinterpret_cast<const u32x4*>(wrow1 + kp);
            acc0 = Lp<T>::mfma(av, b0, acc0);
            acc1 = Lp<T>::mfma(av, b1, acc1);
        }
        // epilogue: adjacent lanes hold adjacent channels of the same pixel; exchanging one register between lane pairs
        // lets every lane store TWO channels (4 bytes) of one pixel: even lanes take pixel-register r, odd lanes r + 1
        const StemTile tl = grid.tile(tile);
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float v0a = fmaxf(acc0[r] + bias0, 0.0f), v0b = fmaxf(acc0[r + 1] + bias0, 0.0f);
            const float v1a = fmaxf(acc1[r] + bias1, 0.0f), v1b = fmaxf(acc1[r + 1] + bias1, 0.0f);
            const float g0 = __shfl_xor(odd ? v0a : v0b, 1, 64);   // even gets partner's value for register r, odd for r + 1
            const float g1 = __shfl_xor(odd ? v1a : v1b, 1, 64);
            const int rr = r + odd;
            const int mm = (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
            const int oy = tl.ty0 + wave * 2 + (mm >> 4), ox = tl.tx0 + (mm & 15);
            const size_t o = (((size_t)tl.view * grid.OH + oy) * grid.OW + ox) * 64 + (n & ~1);
            const unsigned w0 = odd ? Lp<T>::pack2(g0, v0b) : Lp<T>::pack2(v0a, g0);
            const unsigned w1 = odd ? Lp<T>::pack2(g1, v1b) : Lp<T>::pack2(v1a, g1);
            *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(p.out) + o) = w0;
            *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(p.out) + o + 32) = w1;
        }
    });
}

// -----------------------------------------------------------------------------------------------------
// stem of the f32s engine: stem_lp_kernel's layout (K ky-major, 24 slots per patch row, 11 MFMA steps) with BOTH operands as IEEE-half
// hi / lo pairs -- the image patch is split while it is staged (two 16-bit patches), the weights were split and re-laid once by
// stem_relayout_f32s_kernel (two [64][184] tiles, hi at byte 0 and lo at byte STEM_LP_TILE_BYTES of the stem's slot in the pre-split
// blob copy) -- three MFMAs per step and output tile (x_hi w_hi + x_lo w_hi + x_hi w_lo), float32 accumulation, float32 output:
// 66 MFMAs per wave and tile where the exact-fp32 stem_kernel issues 148 at four times the cycles each.
// -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stem_f32s_kernel(StemArgs p) {
    constexpr int PROW = STEM_LP_PROW, KP = STEM_KP, WPITCH = STEM_WPITCH;
    __shared__ __attribute__((aligned(16))) unsigned short patch[2][STEM_LP_PATCH_ELEMS];   // [hi | lo]
    __shared__ __attribute__((aligned(16))) unsigned short wl[2][STEM_LP_TILE_ELEMS];       // [hi | lo]
    const StemGrid grid(p);
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= grid.ntiles) return;

    stem_copy_weights<STEM_F32S_W_BYTES / 1024>(p.w_lp, &wl[0][0], tid);   // both tiles as they lie
    float pv[STEM_NIT][3];
    auto scatter = [&]() {
        stem_scatter<PROW>(tid, pv, [&](int at, const float (&v)[3]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const _Float16 h = (_Float16)v[c];
                patch[0][at + c] = __builtin_bit_cast(unsigned short, h);
                patch[1][at + c] = __builtin_bit_cast(unsigned short, (_Float16)(v[c] - (float)h));
            }
        });
    };
    stem_gather(p, grid, blockIdx.x, tid, pv);
    scatter();
    stem_lp_zero_pads(tid, patch[0], patch[1]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's weight pieces have landed
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, half = lane >> 5;
    const int py = wave * 2 + (m >> 4), px = m & 15;
    const int aoff = (2 * py) * PROW + 6 * px;
    const int n = lane & 31;
    const float bias0 = p.bias[n], bias1 = p.bias[32 + n];
    stem_walk(p, grid, tid, pv, scatter, [&](int tile) {
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KP / 16; ++s) {
            const int kp = 16 * s + 8 * half;
            const int ky = kp / 24, kk = kp % 24;
            u32x4 ah = {0u, 0u, 0u, 0u}, al = {0u, 0u, 0u, 0u};
            if (kp < 168) {
                const unsigned* const aph = reinterpret_cast<const unsigned*>(&patch[0][aoff + ky * PROW + kk]);
                const unsigned* const apl = reinterpret_cast<const unsigned*>(&patch[1][aoff + ky * PROW + kk]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ah[e] = aph[e];
                    al[e] = apl[e];
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f16x8 wh = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(&wl[0][(32 * t + m) * WPITCH + kp]));
                const f16x8 wlo = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(&wl[1][(32 * t + m) * WPITCH + kp]));
                f32x16& acc = t ? acc1 : acc0;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah), wh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, al), wh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah), wlo, acc, 0, 0, 0);
            }
        }
        stem_store<float>(p, grid, tile, lane, wave, acc0, acc1, bias0, bias1);
    });
}

// One-time re-layouts of the stem weights, f32 [148][64] (k = ky*21 + kk) -> [64][184]: cell i of the tile
__device__ __forceinline__ float stem_relayout_cell(const float* __restrict__ w, int i) {
    const int n = i / STEM_WPITCH, kp = i % STEM_WPITCH;
    const int ky = kp / 24, kk = kp % 24;
    float v = 0.0f;
    if (kp < 168 && kk < 21) v = w[(ky * 21 + kk) * 64 + n];
    return v;
}
constexpr int STEM_RELAYOUT_BLOCKS = (STEM_LP_TILE_ELEMS + 255) / 256;   // the grid of both kernels: one thread per cell

// for stem_lp_kernel: one 16-bit tile
template <typename T>
__global__ __launch_bounds__(256) void stem_relayout_kernel(const float* __restrict__ w, unsigned short* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= STEM_LP_TILE_ELEMS) return;
    out[i] = Lp<T>::from_f32(stem_relayout_cell(w, i));
}

// for stem_f32s_kernel: two IEEE-half tiles, hi = rn(w) and lo = rn(w - hi)
__global__ __launch_bounds__(256) void stem_relayout_f32s_kernel(const float* __restrict__ w, unsigned short* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= STEM_LP_TILE_ELEMS) return;
    const float v = stem_relayout_cell(w, i);
    const _Float16 h = (_Float16)v;
    out[i] = __builtin_bit_cast(unsigned short, h);
    out[STEM_LP_TILE_ELEMS + i] = __builtin_bit_cast(unsigned short, (_Float16)(v - (float)h));
}

}  // namespace hgk
