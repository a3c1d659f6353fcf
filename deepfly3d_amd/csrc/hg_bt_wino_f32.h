// fp32 identity-skip bottleneck tail (3x3 -> 1x1 -> + x) with the 3x3 convolution as WINOGRAD F(2x4, 3x3) on the exact-fp32 MFMA
// (round 6: F(2x2, 3x3); round 7: F(2x4, 3x3)).  The exact-fp32 engine sits at the matrix pipe's roof, so the only way left to make it
// faster is to issue fewer MFMAs.  Winograd does a 2 x 4 output patch with 4 x 6 = 24 instead of 72 multiplies per (cin, cout) pair: 3 per
// output pixel (F(2x2): 4, direct: 9) -- the tail's MFMA cycles per tile fall from 2 816 x 64 (direct) to 98 304 (F(2x2)) to 81 920.
//
//   Y = A2^T [ (G2 g G4^T) (.) (B2^T d B4) ] A4      d: 4 x 6 input patch of t1 (per channel), g: 3x3 weights (per cin, cout), Y: 2 x 4 outputs
//
// F(2, 3) down the rows (points 0, 1, -1, inf), F(4, 3) along the columns (points 0, 1, -1, 1/2, -2, inf; the matrices and the numerics gate:
// tests/test_wino24_numerics.py), summed over the 128 input channels INSIDE the transformed domain: 24 "positions" p = (i, j), each a GEMM
//   M_p [128 cout x 16 patches] = U_p [128 cout x 128 cin] . V_p [128 cin x 16 patches]
// over the 16 patches (4 x 4) of an 8 x 16 output tile.  U = G2 g G4^T is transformed once at df3d_hg_set_weights (fp64, rounded once:
// bt_wino_pack_kernel), V = B2^T d B4 costs packed adds / FMAs with exact power-of-two and half-integer coefficients, Y = A2^T M A4 likewise.
//
// Mapping (one workgroup = one 8 x 16 tile, ONE wave per SIMD, v_mfma_f32_16x16x4_f32: 32-cycle issue, 40-cycle dependent latency, so
// consecutive MFMAs always go to different accumulators):
//   * wave w owns output channels 32 w .. 32 w + 31 as two 16-row blocks m, for all 16 patches and all 24 positions: 48 accumulator tiles of
//     4 registers = 192; its output transform is in-lane (lane: patch lane & 15, channels 32 w + 16 m + 4 (lane >> 4) + 0..3);
//   * K is walked in 16 chunks of 8 input channels = 2 K steps s of 4.  Per chunk the four waves build V (24 positions x 8 channels x 16
//     patches = 12 KB, three buffers in LDS) from the t1 halo tile -- lane = (patch, channel, row half h): 18 ds_read_b32, 12 + 20 packed ops,
//     3 ds_write_b128, under the MFMAs of the chunk before -- and each wave then runs 6 passes (s, position pair pp) x 16 MFMAs: B = V_p (one
//     ds_read_b128 = four positions), A = its own 1 KB fragment of U_p straight from global memory (L2-resident, 1.5 MB per bottleneck,
//     requested WN_UBUF - 1 passes = 1 024 MFMA cycles ahead);  ONE barrier per chunk (3 072 MFMA cycles);
//   * t2 = relu(Y + b2) (b2 is the start value of position (1,1), whose column of both A^T is all ones) crosses to the pixel-major mapping
//     of phase 3 through LDS (64 KB in the dead t1 region), and phase 3 is hg_bt_ring_f32.h's, unchanged: W3 through the 4-slot LDS-DMA ring
//     (which takes the dead V buffers' place), residual add, ADD2 / UP / pooled outputs;
//   * in phase 2 every address a chunk needs is complete in ONE register when the chunk's clump ends (round 8, profiles/r08_tail_gaps.txt;
//     scripts/mfma_gaps.py counts what stands between the MFMAs of the built code): the patch columns, with their rows as immediate offsets of
//     the reads, and the store and read bases of V buffer 2, which lies past the 16-bit offset of an LDS access (wn_far_off).  Phase 3's
//     fragment reads are left to hipcc: read one quad ahead through two explicit register sets they measured 0.4-0.8 % SLOWER per launch
//     (the read's latency already hides under the MFMAs in flight; see the record).
//
// U stream: 96 passes x 16 KB.  Passes 0 .. 63 (1 MiB) sit in the block's Winograd slot (p.w2d, in front of W3), passes 64 .. 95 (512 KiB) in the
// block's direct-form stage images (p.wstream, BRF_NSTAGE / L2F_NSTAGE x 8 KB = 832 KB): no launch of an engine with `wino` reads those images
// (hourglass.hip, where they are packed), so the engine's buffer keeps its size.
//
// LDS: V / ring 32 KB | t1 halo tile 90 KB (both 64-channel halves; t2 later) | b3 1 KB = 125 952 B: one workgroup per CU.
// Not bit-identical to the direct form (different products): the engine option `wino` selects it, the tests hold it to the
// fp32 tolerance against the torch oracle on every plan step, and `wino=0` keeps the direct kernels as the bit-identity reference.
#pragma once
#include "hg_bt_common.h"
#include "hg_bt_reg.h"
#include "hg_bt_ring_f32.h"
#include "hg_types.h"

#ifndef WN_ABL
#define WN_ABL 0   // development builds (scripts/build_variant.sh): ablation mask -- phase 2: 1 no U loads, 2 no input transform, 4 no chunk barrier; the rest of a tile: 512 no patch reads, 1024 no V stores, 2048 no packed ops of the input transform; 16 no output transform, 32 no halo DMA for the next tile, 64 no residual / operand loads, 128 no output stores, 256 no phase-3 MFMAs
#endif

namespace hgk {

constexpr int WN_CHUNKS = 16;                          // K chunks of 8 input channels
constexpr int WN_PASSES = 6;                           // per chunk: K step s (4 channels) x position pair pp (8 of the 24 positions)
#ifndef WN_UBUF
#define WN_UBUF 3   // U fragment buffers of a wave (a divisor of WN_PASSES): fragments are requested WN_UBUF - 1 passes ahead (6: hipcc
                    // then moves more accumulators between registers inside the chunk loop)
#endif
constexpr int WN_PASS_BYTES = 4 * 4 * 1024;            // a pass: [wave 4][fragment 4] x 1 KB MFMA A fragments
constexpr int WN_U_BYTES = 64 * WN_PASS_BYTES;         // passes 0 .. 63 in the Winograd slot: 1 MiB per bottleneck
constexpr int WN_U2_BYTES = (WN_CHUNKS * WN_PASSES - 64) * WN_PASS_BYTES;   // passes 64 .. 95 in the direct-form stage images: 512 KiB
constexpr int WN_W3_BYTES = BRF_W3_STAGES * BR_STAGE_BYTES;   // behind U: W3's 16 stage images with their rows permuted (bt_wino_pack_w3_kernel)
constexpr int WN_STREAM_BYTES = WN_U_BYTES + WN_W3_BYTES;
constexpr int WN_STREAM_BYTES_L2 = WN_U_BYTES + 2 * WN_W3_BYTES;   // layer2: U | W3 | Wd (the skip convolution's weights, rows permuted the same way)
constexpr int WN_V_BYTES = 12 * 1024;                  // one V chunk: [K step s 2][position group pg 6][channel k 4][patch slot 16] x 16 bytes
constexpr int WN_T1_OFF = BR_RING_BYTES;               // the W3 ring reuses the V buffers
constexpr int WN_T1_BYTES = 2 * BR_T1_BYTES;           // both 64-channel halves of the 10 x 18 halo tile (92 160)
constexpr int WN_T2_BYTES = BT_TH * BT_TW * 512;       // t2 [128 pixels][128 channels] fp32 (65 536), inside the t1 region
constexpr int WN_B3_OFF = WN_T1_OFF + WN_T1_BYTES;
constexpr int WN_RING2_OFF = WN_B3_OFF + 1024 + 512;   // b3 [256] | b2 [128] | W3 ring slots 4 .. 7
constexpr int WN_LDS_BYTES = WN_RING2_OFF + BR_RING_BYTES;
static_assert(WN_LDS_BYTES <= 160 * 1024, "one workgroup per CU");
constexpr int WN_HALO_K = (BT_HALO / 4 + 3) / 4;            // a wave's halo pieces per 64-channel half (12; the last is wave 0's alone)
static_assert(WN_HALO_K % 4 == 0, "phase 3 requests the halo in four equal parts");
static_assert(WN_PASSES % WN_UBUF == 0 && WN_UBUF >= 2, "a chunk's passes use the same buffers in every chunk");
static_assert(WN_V_BYTES <= BR_RING_BYTES / 2, "V buffers 0, 1 in the W3 ring's slots 0 .. 3, buffer 2 in slots 4 .. 7");
static_assert(WN_T2_BYTES <= WN_T1_BYTES, "t2 lives in the t1 region");
static_assert(WN_U2_BYTES <= BRF_NSTAGE * BR_STAGE_BYTES, "U's second part fits the direct-form stage images");

// Positions: V's position group pg = 3 h + jp holds (row i, column j) = (h ? 3 - a : a, 2 jp + b) in element a + 2 b: row half h of the input
// transform (rows 0, 1 / rows 3, 2 of B2^T d), column pair jp.
__host__ __device__ constexpr int wn_row(int pg, int q4) { return pg >= 3 ? 3 - (q4 & 1) : (q4 & 1); }
__host__ __device__ constexpr int wn_col(int pg, int q4) { return 2 * (pg % 3) + (q4 >> 1); }

// W2' [9][128 cout][128 cin] fp32 (bn3 folded) -> U stream.  One thread per (cout, cin): G2 g G4^T in fp64, each value rounded once.
// Pass P = 6 c + 3 s + pp (chunk c, K step s, position pair pp), wave w, fragment (pgl, m) = 1 KB: lane (r = lane & 15, k = lane >> 4) holds
// U_{pg}[32 w + 16 m + r][8 c + 4 s + k] for the four positions of group pg = 2 pp + pgl (the MFMA A operand of those positions: one float per
// lane).  A wave's four fragments of a pass are 4 KB contiguous: one scalar base, immediate offsets.
__global__ __launch_bounds__(256) void bt_wino_pack_kernel(const float* __restrict__ w2, float* __restrict__ ustream, float* __restrict__ ustream2) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 128 * 128) return;
    const int co = idx >> 7, ci = idx & 127;
    double g[3][3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) g[ky][kx] = (double)w2[((size_t)(ky * 3 + kx) * 128 + co) * 128 + ci];
    double t[4][3];   // G2 g (rows: F(2, 3))
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        t[0][kx] = g[0][kx];
        t[1][kx] = 0.5 * (g[0][kx] + g[1][kx] + g[2][kx]);
        t[2][kx] = 0.5 * (g[0][kx] - g[1][kx] + g[2][kx]);
        t[3][kx] = g[2][kx];
    }
    const int c = ci >> 3, s = (ci >> 2) & 1, k = ci & 3, w = co >> 5, m = (co >> 4) & 1, r = co & 15;
#pragma unroll
    for (int pg = 0; pg < 6; ++pg)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const double* const x = t[wn_row(pg, q4)];
            double u;   // (G2 g) G4^T: columns F(4, 3)
            switch (wn_col(pg, q4)) {
                case 0: u = x[0]; break;
                case 1: u = (x[0] + x[1] + x[2]) / 3.0; break;
                case 2: u = (-x[0] + x[1] - x[2]) / 3.0; break;
                case 3: u = -(16.0 * x[0] + 8.0 * x[1] + 4.0 * x[2]) / 15.0; break;
                case 4: u = (x[0] - 2.0 * x[1] + 4.0 * x[2]) / 15.0; break;
                default: u = x[2]; break;
            }
            const int P = 6 * c + 3 * s + (pg >> 1);
            const size_t off = ((size_t)((P & 63) * 4 + w) * 4 + (pg & 1) * 2 + m) * 256 + (r + 16 * k) * 4 + q4;
            (P < 64 ? ustream : ustream2)[off] = (float)u;
        }
}
// W3 [256][128] fp32 -> 16 stage images (hg_bt_ring_f32.h's: output half nh, 16-float K slice k8; 128 rows x 64 bytes, br_swz) with the ROWS PERMUTED:
// row 32 i + l of an image holds output channel 128 nh + 4 l + i.  Phase 3's accumulator tile i, column l31 is then channel 4 l31 + i: the lane's
// four tiles are four CONSECUTIVE channels of one pixel, and residual, addends, output and pooled outputs move as 16-byte accesses (a quarter of the
// vector-memory instructions, each of which this one-wave-per-SIMD kernel pays for in full; and a wave may have only 64 of them in flight).
__global__ __launch_bounds__(256) void bt_wino_pack_w3_kernel(const float* __restrict__ w3, unsigned char* __restrict__ stream) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= BRF_W3_STAGES * 512) return;
    const int k = idx >> 9, rem = idx & 511, c = rem & 3, r = rem >> 2, nh = k >> 3, k8 = k & 7;
    const int ch = 4 * (r & 31) + (r >> 5);
    *reinterpret_cast<u32x4*>(stream + (size_t)k * BR_STAGE_BYTES + br_swz(r, c)) = *reinterpret_cast<const u32x4*>(w3 + ((size_t)nh * 128 + ch) * 128 + 16 * k8 + 4 * c);
}

// What an instruction costs between two of a wave's fp32 MFMAs when the wave is alone on its SIMD (tests/perf/ubench/mfma_f32_shadow.hip, cycles
// added to a 64-cycle v_mfma_f32_32x32x2_f32): one VALU op 14, a clump of n VALU ops ~10 + 4.3 n (v_pk_add_f32 counts as one), global_load_dwordx4
// with a 64-bit vector address 17.6, with a scalar base + 32-bit lane offset 6.6, LDS-DMA the same, ds_read_b128 2.0, ds_write_b128 3.1, SALU / s_nop 0.
// The exact-fp32 MFMA evidently shares the vector ALU: NOTHING vector hides in its shadow.  Hence, in phase 2: scalar-base loads, the input
// transform as sixteen packed adds in ONE clump, no address arithmetic on the vector side.
// The four U fragments of a pass as ONE inline-assembly statement: scalar base (the wave's 4 KB of the pass), the lane's 16-byte offset, immediate
// offsets.  Inline assembly because, left to hipcc, the loads sink behind the MFMAs that still read the registers it wants to reuse for them (issued
// at the END of the pass they belong to, a vmcnt(1) at the top of every chunk: 580 cycles each); with "=&v" outputs and a scheduling fence behind
// the statement they are issued where they stand.  The s_nop: a base restored from a spill lane by v_readlane right in front of the statement is a
// VALU-writes-SGPR -> VMEM-reads-it hazard (5 wait states) that the hazard recogniser cannot see inside inline assembly (measured: a memory fault).
__device__ __forceinline__ void wn_uload4(f32x4 (&d)[4], const void* sbase, unsigned voff) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:1024\n\t"
                 "global_load_dwordx4 %2, %4, %5 offset:2048\n\tglobal_load_dwordx4 %3, %4, %5 offset:3072"
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3])
                 : "v"(voff), "s"(sbase)
                 : "memory");
}
// ... and the counted wait that makes a pass's four fragments valid (operations retire in issue order: N = the loads issued behind them); it names
// the registers as read-write operands, so the MFMAs that consume them depend on it
template <int N>
__device__ __forceinline__ void wn_uwait(f32x4 (&u)[4]) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]) : "n"(N) : "memory");
}
// An LDS region past the 16-bit immediate offset of an access (V buffer 2): address = lane constant + region offset, the offset as a
// wave-uniform value the compiler cannot fold -- ONE v_add per base, where the source forms it (an s_mov is free beside the MFMAs); folded,
// hipcc forms the address with a literal v_add where it wants it, between two MFMAs
__device__ __forceinline__ unsigned wn_far_off(unsigned off) {
    asm volatile("" : "+s"(off));
    return off;
}
// one 16-byte load, scalar base + lane offset, issued where it stands (the residual tiles: hipcc sinks compiler-visible loads to their first use --
// the epilogue -- and the wave then sits out an HBM round trip with nothing else to do; measured 4.7 % of the kernel)
__device__ __forceinline__ void wn_xload1(f32x4& d, const void* sbase, unsigned voff) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=&v"(d) : "v"(voff), "s"(sbase) : "memory");
}
// four 16-byte loads STEP bytes apart (scalar base + lane offset), issued where they stand
template <int STEP>
__device__ __forceinline__ void wn_xload4s(f32x4 (&d)[4], const void* sbase, unsigned voff) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:%6\n\t"
                 "global_load_dwordx4 %2, %4, %5 offset:%7\n\tglobal_load_dwordx4 %3, %4, %5 offset:%8"
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3])
                 : "v"(voff), "s"(sbase), "n"(STEP), "n"(2 * STEP), "n"(3 * STEP)
                 : "memory");
}

// L2: fp32 layer2 (128 -> 128 -> 128 -> 256 with a 1x1 SKIP CONVOLUTION instead of the identity skip): the same phases 1-2 on its t1, and in
// phase 3 the skip convolution accumulated into the same accumulators behind W3 (as layer2_tail_f32_kernel does): per output half eight more ring
// stages (Wd, rows permuted like W3's) whose A operand is the raw x of the lane's pixel, prefetched from global memory in MFMA layout; no residual.
template <bool UP, bool ADD2 = false, bool L2 = false>
__global__ __launch_bounds__(256, 1) void bottleneck_wino_f32_kernel(BtRingArgs p) {
    static_assert(!(UP && ADD2), "the fused up-path sum is written by plain blocks");
    static_assert(!L2 || (!UP && !ADD2), "layer2 is a plain block");
    using T = float;
    constexpr int CIN = L2 ? 128 : 256, CO = 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const ring = smem;                      // phase 3 (the V double buffer until then)
    unsigned char* const t1_lds = smem + WN_T1_OFF;
    float* const b3_lds = reinterpret_cast<float*>(smem + WN_B3_OFF);
    float* const b2_lds = b3_lds + 256;
    const unsigned ring_addr = lds_addr(ring), t1_addr = lds_addr(t1_lds);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = p.W / BT_TW, tiles_y = p.H / BT_TH;
    const int ntiles = p.V * tiles_y * tiles_x;
    // PERSISTENT: one workgroup per CU walks tiles vb = blockIdx.x, + gridDim.x, ... (a single resident workgroup has nobody to hide its
    // prologue behind: the next tile's t1 halo is requested while this tile's phase 3 runs).  XCD-aware order (hg_bt_common.h bt_tile):
    // virtual block vb runs on XCD vb % 8 (the grid is a multiple of 8, or one tile per workgroup) and XCD x takes the x-th contiguous eighth.
    auto tile_of = [&](int vb, int& tx0, int& ty0, int& view) {
        const BtTile t = bt_tile<BT_TW, BT_TH>(vb, ntiles, tiles_x, tiles_y);
        tx0 = t.tx0, ty0 = t.ty0, view = t.view;
    };
    // the t1 halo tile by LDS-DMA, both 64-channel halves (hg_bt_common.h bt_t1_issue_persistent; half kh at t1 + kh * BR_T1_BYTES)
    // ONE lane-derived register lives across phase 2 (uoff, the U loads' lane offset, opaque to the compiler); whatever else a tile derives from the
    // lane index is recomputed from it where it is needed -- kept alive, `lane` itself sat in scratch and every reload was a vmcnt(0)
    unsigned uoff = (unsigned)(lane * 16);
    asm volatile("" : "+v"(uoff));
    // (k0, k1: the wave's pieces wave + 4 k of k0 <= k < k1 -- phase 3 requests the next tile's halo a few pieces at a time)
    auto t1_issue = [&](auto k0_tag, auto k1_tag, int tx0, int ty0, int view) {
        bt_t1_issue_persistent<BT_HW, BT_HALO, 512, 2, decltype(k0_tag)::value, decltype(k1_tag)::value>(p.t1in, p.zeros, view, tx0, ty0, p.H, p.W, t1_addr, wave, uoff);
    };


    // ---- U fragments straight from global memory (L2) into the MFMA A registers: the wave's four fragments of pass P = 6 c + e (chunk c,
    //      pass e of the chunk) are 4 KB at U + (4 P + wave) 4096 -- passes 64 .. 95 in the second part of the stream (p.wstream).  Rolling
    //      prefetch WN_UBUF - 1 passes ahead: at the start of pass e the registers of the pass before are free and take pass e + WN_UBUF - 1
    //      (of the next chunk past the chunk's last pass) ---------------------------------------------------------------------------------------
    const unsigned char* const ubase = reinterpret_cast<const unsigned char*>(p.w2d) + (size_t)wave * 4096;
    const unsigned char* const ubase2 = reinterpret_cast<const unsigned char*>(p.wstream) + (size_t)wave * 4096 - (size_t)64 * WN_PASS_BYTES;
    auto uload = [&](int c, int e, f32x4 (&dst)[4]) {
        const int P = WN_PASSES * c + e;
        wn_uload4(dst, (P < 64 ? ubase : ubase2) + (size_t)P * WN_PASS_BYTES, uoff);
    };

    // ---- input transform: wave -> (row half h = wave & 1, patch rows 2 (wave >> 1) + {0, 1}); lane -> (patch column pc = lane & 3, channel
    //      te = (lane >> 2) & 3 of channel quad kq = (lane >> 4) & 1, patch row 2 (wave >> 1) + (lane >> 5)): 16 patches x 8 channels x 2 row halves.
    // t1 element (halo pixel hp, channel 64 kh + 4 kq + e) sits at hp * 256 + ((kq ^ swz(hp)) << 4) + 4 e of half kh (br_t1_swz): a read of the 64
    // lanes touches 8 slots x 4 banks twice (the two patch rows: a two-way conflict); chunk c's quads are kq = 2 (c & 7) + {0, 1}: an XOR of
    // the address with (c & 7) << 5.  The lane reads halo rows 2 pr + h + t (t = 0, 1, 2: immediate offsets) of halo columns 4 pc + col.
    const int wh = wave & 1;
    // V chunk image [K step s 2][position group pg 6][channel k 4][patch slot 16] x 16 bytes: patch n of channel k in slot n ^ 4 k (a permuted
    // 256-byte row: the 16 lanes of a store quarter -- four patches x four channels -- hit 16 different slots).  The writer (s, k) = (kq, te)
    // stores groups pg = 3 h + jp; the reader, lane (patch r = lane & 15, channel k = lane >> 4), reads the B operand of four positions.
    // These lane constants (rd: the patch columns' read addresses, vwr, vrd) are derived per tile, at the start of phase 2, from a copy of the
    // lane index the compiler cannot see through: kept alive across the tile loop they would also live across phase 3, where layer2's
    // 64 prefetched x operands leave no room for them (one VGPR went to scratch, its reloads a vmcnt(0) behind the x prefetch)
    unsigned rd[6], vwr, vrd;
    auto lane_consts = [&]() {
        int l = (int)(uoff >> 4);
        asm volatile("" : "+v"(l));
        const int ppc = l & 3, pte = (l >> 2) & 3, pkq = (l >> 4) & 1, ppr = 2 * (wave >> 1) + (l >> 5);
#pragma unroll
        for (int col = 0; col < 6; ++col) {
            const int hx = 4 * ppc + col, hp = (2 * ppr + wh) * BT_HW + hx;
            rd[col] = (unsigned)(hp * 256 + ((pkq ^ (hx & 15)) << 4) + 4 * pte);
        }
        vwr = (unsigned)(((pkq * 6 + 3 * wh) * 4 + pte) * 256 + (((4 * ppr + ppc) ^ (4 * pte)) << 4));
        vrd = (unsigned)((l >> 4) * 256 + (((l & 15) ^ (4 * (l >> 4))) << 4));
    };
    // three V buffers (chunk c is read from buffer c % 3 while chunk c + 2 is built into (c + 2) % 3: a chunk's first fragments can then be
    // requested before the barrier that ends the chunk in front of it): 0, 1 where the W3 ring's slots 0 .. 3 will be, 2 where its slots 4 .. 7 will be
    auto vbuf_off = [](int b) { return b == 0 ? 0 : b == 1 ? BR_RING_BYTES / 2 : WN_RING2_OFF; };
    // Buffer 2 sits past the 16-bit offset of an LDS access from the lane constants (wn_far_off): its store base (vwr2) and fragment read base
    // (vrd2) are formed in the clump of the chunk that needs them first -- not by a v_add where hipcc wants the address, between two MFMAs
    unsigned vrd2 = 0, vwr2 = 0;
    auto vrd_of = [&](int b) { return b == 2 ? smem + vrd2 : smem + vbuf_off(b) + vrd; };
    // the F(2, 3) step of the two rows a lane builds, per column: (t0 - t2, t1 + t2) for h = 0 (rows 0, 1 of B2^T d), (t0 - t2, t1 - t0) for
    // h = 1 (rows 3, 2) -- one form, two packed FMAs with wave-uniform coefficients.  The zero coefficients add 0 * t exactly for every finite
    // t; only a non-finite t1 value would become NaN here instead of staying infinite, and no Winograd form carries an infinity through anyway:
    // every output of A^T M A sums positions in which one infinite input has opposite signs (inf - inf = NaN), and t1 = relu(W1' a + b1) of
    // finite activations is finite
    const f32x2 cw2 = {-1.0f, wh ? 0.0f : 1.0f}, cw0 = {0.0f, wh ? -1.0f : 0.0f};
    float tR[6][3];   // the patch values of the lane's (patch, channel, row half): [column][row]
    unsigned ta[6];   // LDS addresses of the next patch reads (computed in the VALU clump of the chunk before)
    // (the empty asm: the address is complete in ONE register where it is formed -- in the clump -- and rows t = 1, 2 are immediate offsets of
    // the reads; left open, hipcc folds the row offset into the scalar term and forms every row's address with a v_add between two MFMAs)
    auto t_addr = [&](int c) {   // chunk c's patch columns
#pragma unroll
        for (int col = 0; col < 6; ++col) {
            ta[col] = (rd[col] ^ (unsigned)((c & 7) << 5)) + (t1_addr + (unsigned)((c >> 3) * BR_T1_BYTES));
            asm volatile("" : "+v"(ta[col]));
        }
    };
    auto t_read = [&](int col) {   // column col of the lane's three rows
        typedef const __attribute__((address_space(3))) float* lds_f;
        if (WN_ABL & 512) {   // (timing only: no patch reads)
            asm volatile("" : "+v"(tR[col][0]), "+v"(tR[col][1]), "+v"(tR[col][2]));
            return;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) tR[col][t] = *(lds_f)(size_t)(ta[col] + t * BT_HW * 256);
    };
    f32x4 vo[3];   // V of the lane's (patch, channel, row half): column pair jp -> (row a, column 2 jp + b) in element a + 2 b
    auto t_transform = [&](int c_next_addr) {
        f32x2 x[6];
#pragma unroll
        for (int col = 0; col < 6; ++col) {
            const f32x2 P = {tR[col][0], tR[col][1]};
            if (WN_ABL & 2048) {   // (timing only: no packed ops)
                x[col] = P;
                continue;
            }
            x[col] = cw0 * f32x2{tR[col][0], tR[col][0]} + (cw2 * f32x2{tR[col][2], tR[col][2]} + P);
        }
        f32x2 v[6];
        if (WN_ABL & 2048) {
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = x[j];
        } else {   // B4^T along the columns (tests/test_wino24_numerics.py: _bt4_f32)
            const f32x2 h = {0.5f, 0.5f}, two = {2.0f, 2.0f};
            const f32x2 d13 = x[3] - x[1], d24 = x[4] - x[2];
            v[0] = h * d13 + (((x[0] + x[4]) - two * x[2]) + d13);
            v[1] = h * x[3] + (two * x[3] + (h * x[2] + (x[4] - x[1])));
            v[2] = h * x[3] + (((x[4] + x[1]) - two * x[2]) - h * x[2]);
            v[3] = two * (x[3] - x[1]) + d24;
            v[4] = h * (x[1] - x[3]) + d24;
            v[5] = h * d24 + (((x[5] + x[1]) - two * x[3]) + d24);
        }
#pragma unroll
        for (int jp = 0; jp < 3; ++jp) vo[jp] = f32x4{v[2 * jp][0], v[2 * jp][1], v[2 * jp + 1][0], v[2 * jp + 1][1]};
        t_addr(c_next_addr);
    };
    // ... and column pair jp's 16 bytes into V buffer `buf`: in phase 2 one store per MFMA group (between MFMAs an LDS instruction is all but free)
    auto v_store = [&](int buf, int jp) {
        if (WN_ABL & 1024) {   // (timing only: no V stores)
            asm volatile("" ::"v"(vo[jp]));
            return;
        }
        *reinterpret_cast<f32x4*>((buf == 2 ? smem + vwr2 : smem + vbuf_off(buf) + vwr) + jp * 1024) = vo[jp];
    };
    auto t_transform_write = [&](int buf, int c_next_addr) {   // (tile entry: clump, then the stores)
        t_transform(c_next_addr);
#pragma unroll
        for (int jp = 0; jp < 3; ++jp) v_store(buf, jp);
    };
    // W3's 16 stages in two sets of eight (one per 128-channel output half): stage k -> slot k % 8, slots 0 .. 3 where the V buffers were, 4 .. 7
    // in a region of their own.  A whole half is resident before its K loop starts: no wait, no barrier inside the loop (operations retire in
    // issue order, so a wait for a young ring stage would also wait for every older load -- the tile's 128 KB of residual values, the next
    // tile's halo, which all 256 workgroups request within the same microsecond)
    auto ring_slot = [](int k) { return (k & 7) < 4 ? (k & 7) * BR_STAGE_BYTES : WN_RING2_OFF + ((k & 7) - 4) * BR_STAGE_BYTES; };
    auto ring_issue8 = [&](int set) {   // stage set: W3 half 0, W3 half 1 (, L2: Wd half 0, Wd half 1); this wave copies pieces 2 wave, 2 wave + 1 of each stage
        unsigned wvoff = (unsigned)wave * 2048u + uoff;
        asm volatile("" : "+v"(wvoff));   // (per call: not one more register across phase 2)
#pragma unroll
        for (int k = 8 * set; k < 8 * set + 8; ++k)
            br_ring_issue(reinterpret_cast<const unsigned char*>(p.w2d) + WN_U_BYTES, k, ring_addr + (unsigned)ring_slot(k), wave, wvoff);
    };

#ifdef DF3D_BT_TIMING
    unsigned long long stamp_ = __builtin_amdgcn_s_memtime();   // (timing builds: scripts/probe_wino.py)
#endif
    int vb = blockIdx.x;
    int tx0, ty0, view;
    tile_of(vb, tx0, ty0, view);
    t1_issue(std::integral_constant<int, 0>{}, std::integral_constant<int, WN_HALO_K>{}, tx0, ty0, view);
    b3_lds[tid] = L2 ? p.b3[tid] + p.bd[tid] : p.b3[tid];   // (L2: b3 + bd as ONE float add, as the direct kernels)
    if (tid < 128) b2_lds[tid] = p.b2[tid];
    bool first = true;

#pragma unroll 1
    for (;;) {
        const int vbn = vb + (int)gridDim.x;
        const bool has_next = vbn < ntiles;
        int ntx0 = 0, nty0 = 0, nview = 0;
        if (has_next) tile_of(vbn, ntx0, nty0, nview);
        // uniform byte offsets of this wave's two tile rows (full resolution) / its one half-resolution row inside a [V][H][W][256] fp32 tensor
        const size_t ftile = (((size_t)view * p.H + ty0 + 2 * wave) * p.W + tx0) * (CO * 4);
        const size_t htile = (((size_t)view * (p.H / 2) + ty0 / 2 + wave) * (p.W / 2) + tx0 / 2) * (CO * 4);
        const unsigned char* const xtile = reinterpret_cast<const unsigned char*>(p.in) + (L2 ? ftile / 2 : ftile);   // (L2: x has 128 channels)

        // accumulators [position group pg 6][row block m 2][position q4 4] (b2 is added to position (1,1) in the output transform: as a start
        // value it would be a global load straight into accumulator registers, and the wait hipcc puts in front of the first MFMA that touches
        // them sits inside the chunk loop)
        f32x4 acc[48];   // (their first MFMAs take a zero addend: chunk 0, K step 0)
        f32x4 ufr[WN_UBUF][4];
#pragma unroll
        for (int e = 0; e < WN_UBUF - 1; ++e) uload(0, e, ufr[e]);
        // first tile: both t1 halves of this wave have landed once only the loads issued behind them are outstanding.  Later tiles: the halo was
        // requested during the tile before's phase 3, whose counted waits and barriers have long published it.  The barrier: every wave is past
        // its last reads of the ring (the tile before), V buffer 0 may be written
        if (first) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (WN_UBUF - 1)) : "memory");
        first = false;
        br_barrier();
        BR_STAMP(0);
        lane_consts();
        t_addr(0);
#pragma unroll
        for (int col = 0; col < 6; ++col) t_read(col);
        t_transform_write(0, 1);
#pragma unroll
        for (int col = 0; col < 6; ++col) t_read(col);
        t_transform_write(1, 2);
        br_barrier();
        BR_STAMP(1);

        // ---- phase 2: 16 chunks x 6 passes (K step s = e / 3, position pair pp = e % 3) x 4 MFMA groups (position group 2 pp + (g >> 1), row block
        //      g & 1) x 4 positions.  Chunk c: MFMAs on V(c) (buffer c % 3) while V(c + 2) is built.  Nothing vector-side hides behind an fp32
        //      MFMA here, so a chunk issues, beside its 96 MFMAs: 24 U loads (scalar base), 12 + 18 LDS reads, 3 LDS stores, ONE clump of packed
        //      ops, one barrier ------------------------------------------------------------------------------------------------------------------
        f32x4 vf[2][2];
        // c: the chunk (runtime); BR = c % 3 and FIRST = (c == 0) as compile-time tags
        auto chunk = [&](int c, auto br_tag, auto first_tag) {
            constexpr int BR = decltype(br_tag)::value;
            constexpr bool FIRST = decltype(first_tag)::value;
            const int cn = c + 1 < WN_CHUNKS ? c + 1 : c;   // (the last chunks re-request fragments / rebuild buffers nobody reads any more: one code path)
            const int c3 = c + 3 < WN_CHUNKS ? c + 3 : WN_CHUNKS - 1;
            const unsigned char* const vb_ = vrd_of(BR);   // (BR == 2: vrd2, formed in the clump of the chunk before)
            if (FIRST) {
#pragma unroll
                for (int g = 0; g < 2; ++g) vf[0][g] = *reinterpret_cast<const f32x4*>(vb_ + g * 1024);
            }
#pragma unroll
            for (int e = 0; e < WN_PASSES; ++e) {
                const int pp = e % 3;
                __builtin_amdgcn_sched_barrier(0);
                if (!(WN_ABL & 1)) {
                    wn_uwait<4 * (WN_UBUF - 2)>(ufr[e % WN_UBUF]);   // this pass's fragments have landed: behind them only the passes' between
                    const int eu = e + WN_UBUF - 1;   // ... and the registers of the pass before take the fragments of pass e + WN_UBUF - 1
                    if (eu < WN_PASSES) uload(c, eu, ufr[eu % WN_UBUF]);
                    else uload(cn, eu - WN_PASSES, ufr[eu % WN_UBUF]);
                    __builtin_amdgcn_sched_barrier(0);   // (... issued HERE: the scheduler would sink the statement behind the pass's MFMAs)
                }
                if (e == 3) {   // the chunk's one clump
                    if (BR == 0) {   // this chunk's stores go to buffer 2
                        vwr2 = vwr + wn_far_off(WN_RING2_OFF);
                        asm volatile("" : "+v"(vwr2));
                    }
                    if (BR == 1) {   // the next chunk reads buffer 2 (its first fragments in this chunk's last pass)
                        vrd2 = vrd + wn_far_off(WN_RING2_OFF);
                        asm volatile("" : "+v"(vrd2));
                    }
                    if (!(WN_ABL & 2)) {
                        if (WN_ABL & 4096) t_transform_write((BR + 2) % 3, c3);   // (development: the stores right behind the clump)
                        else t_transform(c3);   // V(c + 2) from the patch read in passes 0, 1; addresses for the reads of chunk c + 1's passes 0, 1
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // LDS instructions are all but free between MFMAs: the V fragment reads of the next pass (pass 5: the NEXT chunk's pass 0,
                    // whose buffer was complete a barrier ago), in passes 0, 1 a column of the patch V(c + 2) is built from, in pass 3 a V store
                    if (g < 2) {
                        const int en = e + 1, sn = en / 3, ppn = en % 3;
                        if (e < WN_PASSES - 1) vf[en & 1][g] = *reinterpret_cast<const f32x4*>(vb_ + (sn * 6 + 2 * ppn + g) * 1024);
                        else vf[0][g] = *reinterpret_cast<const f32x4*>(vrd_of((BR + 1) % 3) + g * 1024);
                    }
                    if (e < 2 && g < 3 && !(WN_ABL & 2)) t_read(3 * e + g);
                    if (e == 3 && g < 3 && !(WN_ABL & (2 | 4096))) v_store((BR + 2) % 3, g);
                    const int pgl = g >> 1, m = g & 1, ai = ((2 * pp + pgl) * 2 + m) * 4;
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        if (FIRST && e < 3)   // a tile's first product into each accumulator starts from zero
                            acc[ai + q4] = __builtin_amdgcn_mfma_f32_16x16x4f32(ufr[e % WN_UBUF][2 * pgl + m][q4], vf[e & 1][pgl][q4], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
                        else
                            acc[ai + q4] = __builtin_amdgcn_mfma_f32_16x16x4f32(ufr[e % WN_UBUF][2 * pgl + m][q4], vf[e & 1][pgl][q4], acc[ai + q4], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (!(WN_ABL & 4)) br_barrier();   // V(c) is read by every wave (its buffer is rebuilt two chunks on), V(c + 2) written by every wave
        };
        chunk(0, std::integral_constant<int, 0>{}, std::true_type{});
#pragma unroll 1
        for (int c = 1; c < WN_CHUNKS; c += 3) {
            chunk(c, std::integral_constant<int, 1>{}, std::false_type{});
            chunk(c + 1, std::integral_constant<int, 2>{}, std::false_type{});
            chunk(c + 2, std::integral_constant<int, 0>{}, std::false_type{});
        }
        // the last chunk re-requested fragments nobody multiplies: keep their registers named until they have landed (a load whose destination is
        // dead to the compiler lands, asynchronously, in whatever the register holds by then)
        if (!(WN_ABL & 1)) {
#pragma unroll
            for (int e = 0; e < WN_UBUF - 1; ++e) wn_uwait<0>(ufr[e]);
        }

        BR_STAMP(2);
        // Everything phase 3 derives from the lane index is derived HERE, per tile, from a copy the compiler cannot see through: hoisted out of
        // the tile loop these ~60 lane constants would live across phase 2, where the 256 + 256 registers are spoken for (scratch spills, and
        // every reload a vmcnt(0) in the middle of the asynchronous machinery)
        int lane3 = (int)(uoff >> 4);
        asm volatile("" : "+v"(lane3));
        const int half3 = lane3 >> 5, l31_3 = lane3 & 31;
        const unsigned char* const wf0 = ring + br_swz(l31_3, half3);
        const unsigned char* const wf1 = ring + br_swz(l31_3, 2 + half3);
        const int py = 2 * wave + (l31_3 >> 4), px = l31_3 & 15;   // this wave's 32 pixels (phase 3)
        // phase 3's global addresses = (tile, register)-dependent UNIFORM part + one of two per-lane byte offsets (pixel 4 half / half-resolution
        // pixel 2 half of the register's group, channels 4 l31 .. 4 l31 + 3 -- bt_wino_pack_w3_kernel): scalar address arithmetic, two VGPRs -- not one address register pair per access
        const unsigned lane_full = (unsigned)((4 * half3 * CO + 4 * l31_3) * 4);
        const unsigned lane_half = (unsigned)((2 * half3 * CO + 4 * l31_3) * 4);
        // W3's first half into the ring (both V buffers are dead; slots 4 .. 7 were last read a tile ago): it lands under the output transform
        ring_issue8(0);

        // ---- output transform Y = A2^T M A4, ReLU, t2 -> LDS (pixel-major, 16-byte chunk ch of pixel (y, x) in slot ch ^ (x & 15) ^ ((y >> 1) & 1)
        //      of its 512-byte row, as phase 3 reads it).  Lane: patch (pr, pc) = (r >> 2, r & 3) of r = lane & 15, channels 32 wave + 16 m + 4 q + 0..3
        //      (q = lane >> 4): per (m, output pixel) one 16-byte store ----
        if (WN_ABL & 16) {   // (timing only: one value that depends on every accumulator tile, so that phase 2 stays)
            float keep = 0.0f;
#pragma unroll
            for (int k = 0; k < 48; ++k) keep += acc[k][0];
            *reinterpret_cast<float*>(t1_lds + lane3 * 4) = keep;
        } else {
            const int q3 = lane3 >> 4, opr = (lane3 & 15) >> 2, opc = lane3 & 3;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                f32x4 y[2][4];
                const f32x4 bb = *reinterpret_cast<const f32x4*>(b2_lds + 32 * wave + 16 * m + 4 * q3);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    float M[4][6];
#pragma unroll
                    for (int pg = 0; pg < 6; ++pg)
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) M[wn_row(pg, q4)][wn_col(pg, q4)] = acc[(pg * 2 + m) * 4 + q4][reg];
                    M[1][1] += bb[reg];
                    float s[2][6];   // A2^T M: rows
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        s[0][j] = M[0][j] + M[1][j] + M[2][j];
                        s[1][j] = M[1][j] - M[2][j] - M[3][j];
                    }
#pragma unroll
                    for (int a = 0; a < 2; ++a) {   // ... A4 (tests/test_wino24_numerics.py: _at4_f32)
                        const float sa = s[a][1] + s[a][2], sb = s[a][1] - s[a][2];
                        y[a][0][reg] = br_relu(s[a][0] + sa + s[a][3] + s[a][4]);
                        y[a][1][reg] = br_relu(sb + 0.5f * s[a][3] - 2.0f * s[a][4]);
                        y[a][2][reg] = br_relu(sa + 0.25f * s[a][3] + 4.0f * s[a][4]);
                        y[a][3][reg] = br_relu(sb + 0.125f * s[a][3] - 8.0f * s[a][4] + s[a][5]);
                    }
                }
                const int ch = 8 * wave + 4 * m + q3;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int yy = 2 * opr + a, xx = 4 * opc + b;
                        *reinterpret_cast<f32x4*>(t1_lds + (yy * BT_TW + xx) * 512 + (((ch ^ (xx & 15) ^ (opr & 1)) & 31) << 4)) = y[a][b];
                    }
            }
        }
        BR_STAMP(3);
        br_wait_vm(0);   // the ring's first half (and whatever is older: the tile before's stores, a whole tile ago)
        br_barrier();    // t2 and the eight stages are every wave's
        f32x16 t2[4];
        {
            const unsigned rbase = (unsigned)((py * BT_TW + px) * 512 + ((half3 ^ (px & 15) ^ (wave & 1)) << 4));
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {   // registers 4 g + e of tile m: channels 32 m + 8 g + 4 half + e = chunk 8 m + 2 g + half, in slot chunk ^ f
                    const f32x4 v = *reinterpret_cast<const f32x4*>(t1_lds + (rbase ^ (unsigned)((8 * m + 2 * g) << 4)));
#pragma unroll
                    for (int e = 0; e < 4; ++e) t2[m][4 * g + e] = v[e];
                }
        }

        br_barrier();   // every wave holds its t2 in registers: the t1 region may take the next tile's halo
        const bool halo_next = has_next && !(WN_ABL & 32);
        // ---- What phase 3 reads from memory -- the next tile's t1 halo (92 KB per workgroup), the residual values (and the ADD2 addends / UP values)
        //      of each output half (64 + 16 KB) -- is requested A FEW OPERATIONS AT A TIME between the MFMAs of the K loops (`feed`, below), each
        //      6 000 MFMA cycles or more in front of its first use.  Requested in one burst here (round 8) the 43 operations of a wave took 6 400
        //      cycles to ISSUE: 256 workgroups in step ask for 40 MB within a microsecond, a CU holds some 70 KB of loads in flight, and a
        //      vector-memory instruction that finds the queue full stalls its wave, which has nothing else to run (profiles/r09_tail_queue.txt:
        //      the stamps show the time in the issue, not in any wait).  L2 keeps the halo burst: its x operands are plain loads, and no register
        //      is free across its phase 3 for a second set of halo lane values ----
        if constexpr (L2) {
            if (halo_next) t1_issue(std::integral_constant<int, 0>{}, std::integral_constant<int, WN_HALO_K>{}, ntx0, nty0, nview);
        }
        f32x4 xres[1][16];   // !L2: the CURRENT output half's residual values, [register r <-> pixel (r & 3) + 8 (r >> 2) + 4 half]: channels 128 nh + 4 l31 .. + 3
                             // L2: [0][2 k8 + jj] = the skip convolution's A operand, x[this lane's pixel][16 k8 + 8 jj + 4 half ..]
        f32x4 exv[4];        // ADD2: the addends / UP: the half-resolution values of the current half's four pixel quads
        static_assert(!(UP && ADD2), "one extra operand");
        // (inline assembly: scalar base + lane offset, issued where it stands; a quarter g of output half nh: registers 4 g .. 4 g + 3 = pixels
        // 8 g .. 8 g + 3 (+ 4 half) = row g >> 1, columns 8 (g & 1) .., and the extra operand of pixel quad g.  Half 1 goes into the registers
        // of half 0, which epilogue a has read by then)
        auto res_issue = [&](int nh, int g) {
            if (WN_ABL & 64) {
#pragma unroll
                for (int j = 0; j < 4; ++j) xres[0][4 * g + j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            } else {
                wn_uload4(*reinterpret_cast<f32x4(*)[4]>(&xres[0][4 * g]), xtile + ((size_t)(g >> 1) * p.W + 8 * (g & 1)) * (CIN * 4) + nh * 512, lane_full);
            }
            if constexpr (ADD2 || UP)
                wn_xload1(exv[g], reinterpret_cast<const unsigned char*>(ADD2 ? p.add2 : p.in2) + htile + ((g & 1) + 4 * (g >> 1)) * (CO * 4) + nh * 512, lane_half);
        };
        // W3 stage k8 (2 048 MFMA cycles) of output half nh is about to start.  First half: stages 0 .. 3 take a quarter of the next tile's halo
        // each (3 x 2 LDS-DMA pieces), stages 2 .. 5 a quarter of the half's residual values each -- the halo FIRST, while few of the 64 + 16
        // residual registers are taken: its lane values need a dozen registers, and with every residual register already a load's destination the
        // UP and ADD2 kernels spilled.  The last residual quarter is 6 000 MFMA cycles ahead of its use.  Second half: stages 0 .. 3 take the
        // residual quarters.  A wave's queue therefore holds, in issue order: halo (22, wave 0: 24; none behind the workgroup's last tile),
        // from its third part on interleaved with residual half 0 (16 or 20) | ring set 1 (16) | the stores of epilogue a | residual half 1 |
        // the stores of epilogue b -- the counted waits below follow from that
        auto feed = [&](int nh, int k8) {
            if constexpr (!L2) {
                if (nh == 0 && k8 < 4 && halo_next) {
                    if (k8 == 0) t1_issue(std::integral_constant<int, 0>{}, std::integral_constant<int, WN_HALO_K / 4>{}, ntx0, nty0, nview);
                    if (k8 == 1) t1_issue(std::integral_constant<int, WN_HALO_K / 4>{}, std::integral_constant<int, WN_HALO_K / 2>{}, ntx0, nty0, nview);
                    if (k8 == 2) t1_issue(std::integral_constant<int, WN_HALO_K / 2>{}, std::integral_constant<int, 3 * WN_HALO_K / 4>{}, ntx0, nty0, nview);
                    if (k8 == 3) t1_issue(std::integral_constant<int, 3 * WN_HALO_K / 4>{}, std::integral_constant<int, WN_HALO_K>{}, ntx0, nty0, nview);
                }
                const int g = nh == 0 ? k8 - 2 : k8;
                if (g >= 0 && g < 4) res_issue(nh, g);
            }
        };
        auto res_wait = [&](auto n_tag) {   // the counted wait that makes them valid, naming the registers (the epilogue's reads depend on it)
            constexpr int N = decltype(n_tag)::value;
#pragma unroll
            for (int g = 0; g < 4; ++g) wn_uwait<N>(*reinterpret_cast<f32x4(*)[4]>(&xres[0][4 * g]));
            if constexpr (ADD2 || UP) wn_uwait<N>(exv);
        };
        if constexpr (L2) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                xres[0][r] = *reinterpret_cast<const f32x4*>(xtile + (8 * r) * 4 + (unsigned)((((l31_3 >> 4) * p.W + (l31_3 & 15)) * CIN + 4 * half3) * 4));
        }
        BR_STAMP(4);
        // ---- phase 3: out = W3 relu(t2) + b3 + x  (bottleneck_ring_f32_kernel's exact-fp32 form: rows = the wave's pixels, columns = channels);
        //      L2: out = W3 relu(t2) + Wd x + (b3 + bd) ----
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
            f32x16 o[4];
            if (nh == 1) {
                // the second half's stages were requested behind the first half's K loop(s); younger than them are exactly the first half's
                // epilogue's operations, which need not have drained (operations retire in issue order, and vmcnt counts stores): its 16 output
                // stores and 4 more per pooled output the block writes (pool, pool_in) -- the second half's residual loads come behind this wait.
                // The pooled outputs are the launch's (wave-uniform): one of three immediates; counted without them (round 8) the wait sat out the
                // round trip of the epilogue's first 4 or 8 stores.  Older than ring set 1, hence complete behind this wait and published by the
                // barrier: the next tile's halo
                constexpr int young = 16;
                const int pooled = (p.pool ? 1 : 0) + (!UP && !L2 && p.pool_in ? 1 : 0);
                if (pooled == 0) br_wait_vm(young);
                else if (pooled == 1) br_wait_vm(young + 4);
                else br_wait_vm(young + 8);
                br_barrier();
                BR_STAMP(10);   // (the wait for ring set 1 on its own: stamp 7 is then the K loop alone)
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float bias = b3_lds[nh * 128 + 4 * l31_3 + i];
#pragma unroll
                for (int r = 0; r < 16; ++r) o[i][r] = bias;
            }
            // eight resident stages, no wait, no barrier: stage k8 = the 16-float K slice 16 k8 .. of W3 (operand: registers 8 q2 + 4 jj + e of t2
            // tile k8 >> 1 = channels 32 tile + 16 q2 + 8 jj + 4 half + e) or of Wd (operand: x of the lane's pixel, channels 16 k8 + 8 jj + 4 half + e)
            auto kloop = [&](auto skip_tag) {
                constexpr bool SKIP = decltype(skip_tag)::value;
#pragma unroll
                for (int k8 = 0; k8 < 8; ++k8) {
                    const int tile = k8 >> 1, q2 = k8 & 1;
                    if constexpr (!SKIP) feed(nh, k8);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const f32x4 wf = *reinterpret_cast<const f32x4*>((jj ? wf1 : wf0) + ring_slot(k8) + i * 2048);
                            if (WN_ABL & 256) {
                                o[i][0] += wf[0];
                                continue;
                            }
                            if constexpr (SKIP) {
                                const f32x4 xa = xres[0][2 * k8 + jj];
                                mfma_quad<T>(xa[0], xa[1], xa[2], xa[3], wf, o[i]);
                            } else {
                                mfma_quad<T>(t2[tile][8 * q2 + 4 * jj], t2[tile][8 * q2 + 4 * jj + 1], t2[tile][8 * q2 + 4 * jj + 2], t2[tile][8 * q2 + 4 * jj + 3], wf, o[i]);
                            }
                        }
                }
            };
            kloop(std::false_type{});
            if constexpr (L2) {
                br_barrier();             // every wave is through W3's eight stages
                ring_issue8(2 + nh);      // Wd of this half (L2-resident: the one exposed round trip of the half)
                br_wait_vm(0);
                br_barrier();
                kloop(std::true_type{});
            }
            if (nh == 0) {
                br_barrier();     // every wave is through the first half's stages
                ring_issue8(1);   // ... the second half's land under the epilogue
            }
            BR_STAMP(5 + 2 * nh);
            if constexpr (!L2) {
                if (!(WN_ABL & 64)) {
                    // younger than residual half 0: the sixteen stage pieces just requested (the halo is older); than half 1: nothing
                    if (nh == 0) res_wait(std::integral_constant<int, 16>{});
                    else res_wait(std::integral_constant<int, 0>{});
                }
            }
            if (nh == 0) BR_STAMP(9);   // (the wait for residual half 0 on its own: stamp 6 is then the epilogue alone)
            // epilogue: D[row = pixel (r&3) + 8(r>>2) + 4 half of the wave][col = channel nh*128 + 4 l31 + i]: register r of the four tiles = four
            // consecutive channels of one pixel
            // -- walked by 2x2 pixel quads (registers r0, r0 + 1, r0 + 8, r0 + 9: horizontal neighbour r ^ 1, vertical r ^ 8; one half-resolution pixel),
            // so that only four 16-byte values are alive at a time and the max-pools stay inside the lane
#pragma unroll
            for (int key = 0; key < 4; ++key) {
                const int r0 = 2 * (key & 1) + 4 * (key >> 1);
                const int hoff = ((key & 1) + 4 * (key >> 1)) * (CO * 4) + nh * 512;   // the quad's half-resolution pixel (+ 2 half in the lane offset)
                f32x4 xv[4], ov[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) xv[t] = L2 ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : xres[0][r0 + (t & 1) + 8 * (t >> 1)];
                if constexpr (UP) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) xv[t] += exv[key];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int r = r0 + (t & 1) + 8 * (t >> 1);
                    ov[t] = f32x4{o[0][r], o[1][r], o[2][r], o[3][r]};
                    if constexpr (!L2) ov[t] += xv[t];
                    if constexpr (ADD2) ov[t] += exv[key];   // a second fp32 add, as upadd_kernel would have done on the stored tensor
                    const int pl0 = (r & 3) + 8 * (r >> 2);
                    if (!(WN_ABL & 128) || ov[t][0] == 12345.678f)
                        *reinterpret_cast<f32x4*>(reinterpret_cast<unsigned char*>(p.out) + ftile + ((size_t)(pl0 >> 4) * p.W + (pl0 & 15)) * (CO * 4) + nh * 512 + lane_full) = ov[t];
                }
                auto max4 = [](const f32x4 (&v)[4]) {
                    f32x4 m;
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[e] = fmaxf(fmaxf(v[0][e], v[1][e]), fmaxf(v[2][e], v[3][e]));
                    return m;
                };
                if constexpr (!UP && !L2) if (p.pool_in)   // 2x2 max-pool of the block's INPUT (the skip values just added)
                    *reinterpret_cast<f32x4*>(reinterpret_cast<unsigned char*>(p.pool_in) + htile + hoff + lane_half) = max4(xv);
                if (p.pool) *reinterpret_cast<f32x4*>(reinterpret_cast<unsigned char*>(p.pool) + htile + hoff + lane_half) = max4(ov);
            }
            BR_STAMP(6 + 2 * nh);
        }
        if (!has_next) break;
        vb = vbn;
        tx0 = ntx0;
        ty0 = nty0;
        view = nview;
    }
}

}  // namespace hgk
