// What the kernels that stream weights through the LDS-DMA ring share (hg_bt_ring*.h, hg_c1_*.h, hg_l1_*.h, hg_bt_l1.h, hg_bt_wino_f32.h, the ring
// parts of hg_head.h): stage-image and t1-tile geometry, the XCD-aware tile walk, the stage request, the t1 halo tile by LDS-DMA, the t2 start
// values.  Every piece is __forceinline__, and a kernel that calls one compiles to the instructions it had with the piece written out in its body.
// That rule decides what is here: these kernels sit at their register limits and hipcc's schedule follows the order in which the source forms its
// values, so where a shared piece moved one instruction the kernel keeps its own text and says so (DESIGN.md "Where the device code lives").
#pragma once
#include "hg_bt_reg.h"
#include "hg_types.h"

namespace hgk {

constexpr int BR_STAGE_BYTES = 8192;                     // 128 rows x 64 bytes (32 bf16 or 16 floats of K)
constexpr int BR_RING = 4;
constexpr int BR_RING_BYTES = BR_RING * BR_STAGE_BYTES;
constexpr int BR_T1_PITCH = 128 * 2;                    // bytes per halo pixel of the t1 tile: no padding, 16-byte chunks XOR-swizzled
constexpr int BR_T1_BYTES = BT_HALO * BR_T1_PITCH;      // 46 080 (the 12 pad rows of the sixth MFMA row tile are not stored)
// chunk k (8 channels) of halo pixel hp sits in 16-byte slot k ^ ((hp % 18) & 15) of its 256-byte row: the 16 lanes of a
// ds_read_b128 lane group read 16 different tile columns, hence 16 different slots
__device__ __forceinline__ int br_t1_swz(int hp) { return (hp % BT_HW) & 15; }
// stage image: byte offset of 16-byte chunk c of row r (hg_bt_ring.h's header)
__host__ __device__ constexpr int br_swz(int r, int c) { return (r >> 2) * 256 + (((((r & 3) << 2) | c) ^ ((r >> 3) & 3)) << 4); }
// workgroup barrier that does NOT drain the vector-memory queue (a __syncthreads() beside pending LDS-DMA waits vmcnt(0))
__device__ __forceinline__ void br_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// max(x, 0) without the NaN-canonicalising v_max hipcc puts in front of fmaxf on MFMA results: as a signed integer a negative
// float is negative, so v_max_i32(bits, 0) is the ReLU (-0 -> +0).  A builtin, not inline assembly -- see br_relu_pk.
__device__ __forceinline__ float br_relu(float x) {
    const int b = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, b > 0 ? b : 0);
}

// XCD-aware tile order (speed only): workgroup id runs on XCD id % 8, so XCD x takes the x-th contiguous eighth of the n blocks and the workgroups
// resident on it work on neighbouring tiles, whose halos then meet in that XCD's L2.  A bijection of [0, n) for any n.  I: unsigned (blockIdx.x)
// or int (a persistent kernel's virtual block id): the shift is the one that type takes.
template <typename I>
__device__ __forceinline__ int bt_xcd_block(I id, int n) {
    const int xcd = id & 7, q = n >> 3, r = n & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}
struct BtTile { int tx0, ty0, view; };   // first output pixel of the tile, its view
// block id of n -> tile of TW x TH output pixels.  Non-persistent kernels: (blockIdx.x, gridDim.x); persistent ones: (virtual block id, ntiles).
template <int TW, int TH, typename I>
__device__ __forceinline__ BtTile bt_tile(I id, int n, int tiles_x, int tiles_y) {
    const int b = bt_xcd_block(id, n), tx0 = (b % tiles_x) * TW, by = b / tiles_x;
    return BtTile{tx0, (by % tiles_y) * TH, by / tiles_y};
}

// Stage `stage` of a weight stream (8 KB stage images) into the LDS slot at slot_addr: this wave copies pieces 2 wave, 2 wave + 1
// (wvoff = wave * 2048 + lane * 16).  Which stage and which slot is the calling kernel's rule.  Forms the source address, then the destination.
__device__ __forceinline__ void br_ring_issue(const void* stream, int stage, unsigned slot_addr, int wave, unsigned wvoff) {
    br_glds_stage(reinterpret_cast<const unsigned char*>(stream) + (size_t)stage * BR_STAGE_BYTES, wvoff, slot_addr + (unsigned)wave * 2048);
}

// The t1 halo tile by LDS-DMA.  t1 = relu(W1' relu(bn1 x) + b1') was written to HBM for every pixel; a tile's halo (HW pixels wide, HALO pixels, ROWB bytes per pixel in
// memory) arrives one 64-channel half at a time.  Piece pc (1 KB) = halo pixels 4 pc .. 4 pc + 3, lane -> (pixel 4 pc + (lane >> 4), slot
// lane & 15), fetching chunk slot ^ swizzle(pixel) of that pixel's 256-byte half row; halo pixels outside the image fetch from a page of zeros
// (the 3x3 convolution's padding); this wave copies pieces wave, wave + 4, ...
// Two forms of one map.  The direct tails' (two workgroups per CU): a 64-bit address per piece; tin = the view's t1, koff = 256 x the half.
// Called from a lambda that captures tile and lane by reference, and takes them so: by value hipcc knows more of them and divides by HW in 16 bits.
template <int HW, int HALO, int ROWB>
__device__ __forceinline__ void bt_t1_issue(const unsigned char* tin, const void* zeros, const int& tx0, const int& ty0, const int& H, const int& W, int koff,
                                            unsigned t1_addr, const int& wave, const int& lane) {
#ifdef BRF_NO_T1DMA   // development builds: the tails without their t1 halo DMA (what that traffic and its exposed latency cost)
    return;
#endif
#pragma unroll
    for (int k = 0; k < (HALO / 4 + 3) / 4; ++k) {
        const int pc = wave + 4 * k;
        if (pc < HALO / 4) {
            const int hp = 4 * pc + (lane >> 4);
            const int hy = hp / HW, hx = hp % HW;
            const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
            const bool ok = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const unsigned chunk = (unsigned)((lane & 15) ^ ((hp % HW) & 15));
            const unsigned char* const src = ok ? tin + ((size_t)y * W + x) * ROWB + koff + chunk * 16 : reinterpret_cast<const unsigned char*>(zeros) + chunk * 16;
            br_glds_piece64(src, t1_addr + (unsigned)pc * 1024u);
        }
    }
}
// The persistent Winograd kernels' (one workgroup per CU, no register to spare across phase 2): NH halves per call (half h at t1_addr +
// h * HALO * 256), a 32-bit in-view offset (a view's t1 is < 4 GB) and ONE 64-bit add per piece.  The per-piece lane values (halo pixel,
// swizzled chunk) and the per-piece uniform values (piece index, LDS address) are recomputed at every call from uoff = lane * 16, the one
// lane-derived register those kernels keep: hoisted out of the tile loop they are ~70 registers and ~50 spill lanes alive across phase 2 (the
// empty asms hide their loop invariance).  An instruction between fp32 MFMAs or a live VGPR more is measurable in those kernels, which is why
// they do not share the form above.
// K0, K1: the call requests the wave's pieces wave + 4 k of k = K0 .. K1 - 1 only (all of them by default).  A tile's halo in several calls is
// how the fp32 Winograd tails meter it out between the MFMAs of a K loop, instead of one burst that fills the CU's memory queue.
template <int HW, int HALO, int ROWB, int NH, int K0 = 0, int K1 = (HALO / 4 + 3) / 4>
__device__ __forceinline__ void bt_t1_issue_persistent(const void* t1in, const void* zeros, int view, int tx0, int ty0, int H, int W, unsigned t1_addr,
                                                       int wave, unsigned uoff) {
    static_assert(NH == 1 || NH == 2, "one 64-channel half, or both");
    static_assert(0 <= K0 && K0 < K1 && K1 <= (HALO / 4 + 3) / 4, "a range of the wave's pieces");
    int lane_ = (int)(uoff >> 4);
    asm volatile("" : "+v"(lane_));
    int wave_ = wave;
    asm volatile("" : "+s"(wave_));
    const unsigned char* const tin = reinterpret_cast<const unsigned char*>(t1in) + (size_t)view * H * W * ROWB;
    const unsigned char* const zer = reinterpret_cast<const unsigned char*>(zeros);
    const int q = lane_ >> 4, slot = lane_ & 15;
    // the lane's halo pixel (hy, hx): divided by HW once, for the wave's first piece; from piece to piece it advances by 16 halo pixels, which
    // wraps at most once (HW >= 16).  Both halves of a piece share address and bounds test: the second is 256 bytes on (inside the image)
    static_assert(HW >= 16, "one wrap per step of 16 halo pixels");
    const int hp0 = 4 * (wave_ + 4 * K0) + q;
    int hy = hp0 / HW, hx = hp0 - hy * HW;
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        const int pc = wave_ + 4 * k;
        if (pc < HALO / 4) {
            const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
            const bool ok = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const unsigned c16 = (unsigned)((slot ^ (hx & 15)) << 4);
            const unsigned in_view = (unsigned)((y * W + x) * ROWB) + c16;
            const unsigned char* const src = (ok ? tin : zer) + (ok ? in_view : c16);
            br_glds_piece64(src, t1_addr + (unsigned)(pc * 1024));
            if constexpr (NH == 2) br_glds_piece64(src + (ok ? 256u : 0u), t1_addr + (unsigned)(HALO * 256 + pc * 1024));
        }
        hx += 16;
        if (hx >= HW) {
            hx -= HW;
            ++hy;
        }
    }
}

// t2^T accumulators start at b2' (register 4 q + e of tile m <-> channel 32 m + 8 q + 4 half + e); b2 in global memory or in LDS
template <int NT>
__device__ __forceinline__ void bt_t2_start(const float* b2, int half, f32x16 (&t2)[NT]) {
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(b2 + 32 * m + 8 * q + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) t2[m][4 * q + e] = bb[e];
        }
}
}  // namespace hgk
