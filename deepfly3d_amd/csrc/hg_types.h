// What every device header of the stacked-hourglass engine builds on: vector types, the 16-bit storage formats (Lp<T>), element sizes
// (Elem<T>), the input BatchNorm + ReLU on a chunk (PreactCoef), the F32S split-product helpers with their MFMA wrappers, and the
// LDS-DMA / wait-count primitives (lds_addr, br_glds_*, br_wait_vm).
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <type_traits>

namespace hgk {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// The 16-bit storage formats of the low-precision engines.  Both carry a sign, so one bit pattern trick serves both (ReLU and
// max as signed 16-bit integers: br_relu_pk, bf16x2_key); both multiply on the matrix cores at the same rate with fp32
// accumulation.  What differs is where the 16 bits go:
//   __hip_bfloat16  8 exponent bits (fp32's range), 8 significant bits: every stored value carries 2^-9 relative rounding
//   _Float16        IEEE half: 11 significant bits (2^-12 relative, eight times finer), range 6.1e-5 .. 65 504 -- ample for
//                   this network's batch-normalised activations and O(1) weights
// Conversions round to nearest even through the hardware converters (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 on gfx950).
template <typename T>
struct Lp;
template <>
struct Lp<__hip_bfloat16> {
    static __device__ __forceinline__ float to_f32(unsigned short b) { return __uint_as_float(((unsigned)b) << 16); }
    static __device__ __forceinline__ unsigned short from_f32(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
    static __device__ __forceinline__ unsigned pack2(float lo, float hi) {
        const f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    }
    static __device__ __forceinline__ f32x16 mfma(const u32x4& a, const u32x4& b, const f32x16& acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
};
template <>
struct Lp<_Float16> {
    static __device__ __forceinline__ float to_f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
    static __device__ __forceinline__ unsigned short from_f32(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
    static __device__ __forceinline__ unsigned pack2(float lo, float hi) {
        const f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
    }
    static __device__ __forceinline__ f32x16 mfma(const u32x4& a, const u32x4& b, const f32x16& acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    }
};
// 16-byte global store of an activation chunk; HG_NT_STORES (development switch, default 0) makes it a streaming (nt) store in the stack
// heads and the 16-bit layer1 kernel, as the ring bottleneck's MODE 2 does (hg_bt_ring.h: -1.2 % there)
#ifndef HG_NT_STORES
#define HG_NT_STORES 0
#endif
using hg_u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
__device__ __forceinline__ void hg_store16(void* dst, hg_u32x4 v) {
#if HG_NT_STORES
    asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(v) : "memory");
#else
    *reinterpret_cast<hg_u32x4*>(dst) = v;
#endif
}

// eight consecutive floats -> one 16-byte MFMA operand chunk
template <typename T>
__device__ __forceinline__ u32x4 lp_pack8(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    return u32x4{Lp<T>::pack2(a0, a1), Lp<T>::pack2(a2, a3), Lp<T>::pack2(a4, a5), Lp<T>::pack2(a6, a7)};
}

template <typename T>
struct Elem;
template <>
struct Elem<float> {
    static constexpr int BYTES = 4;
    static constexpr int PER16 = 4;  // elements per 16-byte chunk
};
// "f32s" (round 5): float32 STORAGE everywhere -- the fp32 engine's tensors, weights, streams, LDS images and kernels, bit for bit --
// with every product formed on the 16-bit matrix pipe as a two-way IEEE-half split (mfma_chunk<F32S>).  A tag type: sizeof == 4 sends it
// down the float32 path of every helper and kernel; only the MFMA differs.
struct F32S {
    float v;
};
template <>
struct Elem<F32S> {
    static constexpr int BYTES = 4;
    static constexpr int PER16 = 4;
};
template <>
struct Elem<__hip_bfloat16> {
    static constexpr int BYTES = 2;
    static constexpr int PER16 = 8;
};
template <>
struct Elem<_Float16> {
    static constexpr int BYTES = 2;
    static constexpr int PER16 = 8;
};

// Input BatchNorm + ReLU, y = max(x*s + t, 0), on one 16-byte chunk of channels starting at channel c.
// Split in two so the scale/shift loads can be issued with the prefetch (PreactCoef::load) and the arithmetic
// happens after the MFMAs of the current step (preact_apply).
template <typename T>
struct PreactCoef {
    static constexpr int N = Elem<T>::PER16 / 4;  // float4 groups: 1 (f32) or 2 (bf16)
    f32x4 s[N], t[N];
    __device__ __forceinline__ void load(const float* __restrict__ scale, const float* __restrict__ shift, int c) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            s[i] = *reinterpret_cast<const f32x4*>(scale + c + 4 * i);
            t[i] = *reinterpret_cast<const f32x4*>(shift + c + 4 * i);
        }
    }
};

template <typename T>
__device__ __forceinline__ u32x4 preact_apply(u32x4 raw, const PreactCoef<T>& k) {
    if constexpr (sizeof(T) == 4) {
        f32x4 v = __builtin_bit_cast(f32x4, raw);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(fmaf(v[i], k.s[0][i], k.t[0][i]), 0.0f);
        return __builtin_bit_cast(u32x4, v);
    } else {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float lo = Lp<T>::to_f32((unsigned short)(raw[i] & 0xffffu));
            const float hi = Lp<T>::to_f32((unsigned short)(raw[i] >> 16));
            const float a = fmaxf(fmaf(lo, k.s[i >> 1][(2 * i) & 3], k.t[i >> 1][(2 * i) & 3]), 0.0f);
            const float b = fmaxf(fmaf(hi, k.s[i >> 1][(2 * i + 1) & 3], k.t[i >> 1][(2 * i + 1) & 3]), 0.0f);
            o[i] = Lp<T>::pack2(a, b);
        }
        return o;
    }
}

// float32 x -> IEEE-half (hi, lo) with x = hi + lo to 2^-22 |x|: hi = rn(x), lo = rn(x - hi) (the difference is exact in float32).  gfx950's
// v_mfma_f32_32x32x16_f16 keeps subnormal inputs (tests/perf/ubench/mfma_f16_denorm.hip), so lo needs no scaling for small |x|; |x| up to the
// half range 65 504 (the hourglass' batch-normalised activations and O(1) weights are nowhere near it).  Two floats per call: packed converters.
__device__ __forceinline__ void f32s_split2(float x0, float x1, unsigned& hi, unsigned& lo) {
    const f32x2 v = {x0, x1};
    const f16x2 h = __builtin_convertvector(v, f16x2);
    const f32x2 r = {x0 - (float)h[0], x1 - (float)h[1]};
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}

// ---- F32S: float32 products on the half-precision matrix pipe (round 5) ---------------------------------------------------------------
// A lane's share of one 16-float K step is EIGHT floats: the step's 16-byte chunks `half` and `2 + half` (every float32 kernel reads them as
// fragment j = 0 and j = 1 of the step).  With x = hi + lo (f32s_split2: two IEEE halves, x to 2^-22 |x|) the step's product is three K = 16
// half-precision MFMAs -- w_hi x_hi + w_lo x_hi + w_hi x_lo, float32 accumulation; the w_lo x_lo term (2^-22 of the product) is dropped --
// where the exact-fp32 v_mfma_f32_32x32x2_f32 takes eight: 96 matrix-pipe cycles instead of 512.
//   * WEIGHTS are stored pre-split (f32s_presplit_kernel at df3d_hg_set_weights: the blob's copy, from which every stream / LDS image is then
//     packed -- the packers move whole chunks and keep a chunk's index inside its step): per 64-byte step of a row, chunk 0 = hi(f0..3, f8..11),
//     chunk 1 = hi(f4..7, f12..15), chunk 2 = lo(f0..3, f8..11), chunk 3 = lo(f4..7, f12..15) -- so the fragment a lane reads at j = 0 IS the
//     MFMA operand w_hi of its eight K values and the one at j = 1 is w_lo: no arithmetic, no register moves.
//   * ACTIVATIONS are split where they are used, once per fragment pair (make_xpair), however many weight fragments the pair then meets.
__global__ __launch_bounds__(256) void f32s_presplit_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t nsteps) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < nsteps; i += (size_t)gridDim.x * 256) {
        f32x4 f[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = __builtin_bit_cast(f32x4, src[4 * i + c]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // lane half h owns floats 4 h .. 4 h + 3 and 8 + 4 h .. 8 + 4 h + 3 of the step
            unsigned hi[4], lo[4];
            f32s_split2(f[h][0], f[h][1], hi[0], lo[0]);
            f32s_split2(f[h][2], f[h][3], hi[1], lo[1]);
            f32s_split2(f[2 + h][0], f[2 + h][1], hi[2], lo[2]);
            f32s_split2(f[2 + h][2], f[2 + h][3], hi[3], lo[3]);
            dst[4 * i + h] = u32x4{hi[0], hi[1], hi[2], hi[3]};
            dst[4 * i + 2 + h] = u32x4{lo[0], lo[1], lo[2], lo[3]};
        }
    }
}

// the activation operand of one K step: float / 16-bit kernels keep the two chunks as loaded; F32S holds a = the hi halves, b = the lo halves
template <typename T>
struct XPair {
    u32x4 a, b;
};
template <typename T>
__device__ __forceinline__ XPair<T> make_xpair(const u32x4& x0, const u32x4& x1) {
    if constexpr (std::is_same<T, F32S>::value) {
        const f32x4 f0 = __builtin_bit_cast(f32x4, x0), f1 = __builtin_bit_cast(f32x4, x1);
        unsigned hi[4], lo[4];
        f32s_split2(f0[0], f0[1], hi[0], lo[0]);
        f32s_split2(f0[2], f0[3], hi[1], lo[1]);
        f32s_split2(f1[0], f1[1], hi[2], lo[2]);
        f32s_split2(f1[2], f1[3], hi[3], lo[3]);
        return XPair<T>{u32x4{hi[0], hi[1], hi[2], hi[3]}, u32x4{lo[0], lo[1], lo[2], lo[3]}};
    } else {
        return XPair<T>{x0, x1};
    }
}
template <typename T>
__device__ __forceinline__ XPair<T> make_xpair(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    return make_xpair<T>(__builtin_bit_cast(u32x4, f32x4{a0, a1, a2, a3}), __builtin_bit_cast(u32x4, f32x4{a4, a5, a6, a7}));
}

// one 16-byte A fragment x one 16-byte B fragment -> accumulate into a 32x32 tile (float32: K = 8, 16-bit: K = 16)
template <typename T>
__device__ __forceinline__ void mfma_chunk(const u32x4& a, const u32x4& b, f32x16& acc) {
    static_assert(!std::is_same<T, F32S>::value, "F32S kernels multiply whole K steps (mfma_pair): a single pre-split weight chunk is half an operand");
    if constexpr (sizeof(T) == 4) {
        const f32x4 af = __builtin_bit_cast(f32x4, a);
        const f32x4 bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[i], acc, 0, 0, 0);
    } else {
        acc = Lp<T>::mfma(a, b, acc);
    }
}

// one K step: the weight fragments w0 (j = 0), w1 (j = 1) against the activation pair.  W_FIRST: the weights are the MFMA's first operand
// (rows of the result = weight rows).  float / 16-bit: chunk 0 then chunk 1, as the kernels did before round 5.
template <typename T, bool W_FIRST = true>
__device__ __forceinline__ void mfma_pair(const u32x4& w0, const u32x4& w1, const XPair<T>& x, f32x16& acc) {
    if constexpr (std::is_same<T, F32S>::value) {
        const f16x8 WH = __builtin_bit_cast(f16x8, w0), WL = __builtin_bit_cast(f16x8, w1), XH = __builtin_bit_cast(f16x8, x.a), XL = __builtin_bit_cast(f16x8, x.b);
        if constexpr (W_FIRST) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(WH, XH, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(WL, XH, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(WH, XL, acc, 0, 0, 0);
        } else {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(XH, WH, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(XH, WL, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(XL, WH, acc, 0, 0, 0);
        }
    } else if constexpr (W_FIRST) {
        mfma_chunk<T>(w0, x.a, acc);
        mfma_chunk<T>(w1, x.b, acc);
    } else {
        mfma_chunk<T>(x.a, w0, acc);
        mfma_chunk<T>(x.b, w1, acc);
    }
}

// four K = 2 steps of the exact-fp32 engine whose operands sit in registers as scalars (an accumulator row used as the next product's operand):
// acc += sum_e a_e x w[e] with the a's as the MFMA's A operand (A_FIRST) or its B operand.  (F32S sites build an XPair from the eight registers
// of a K step and call mfma_pair.)
template <typename T, bool A_FIRST = true>
__device__ __forceinline__ void mfma_quad(float a0, float a1, float a2, float a3, const f32x4& w, f32x16& acc) {
    static_assert(std::is_same<T, float>::value, "exact-fp32 form");
    const f32x4 a = {a0, a1, a2, a3};
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = A_FIRST ? __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], w[e], acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], a[e], acc, 0, 0, 0);
}

// the LDS byte address of a pointer into __shared__ memory (what M0 takes as an LDS-DMA destination)
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)p; }

// LDS-DMA of one 8 KB stage: this wave's two 1 KB pieces (lane l's 16 bytes land at dst + 16 l; dst wave-uniform, in M0).
// sbase (uniform) + voff (per lane, 32 bit) is the source address.  The instruction's immediate offset is added to the
// global address AND to the LDS address, so the second piece needs no second M0 value.  M0 is saved and restored inside
// the statement.
__device__ __forceinline__ void br_glds_stage(const void* sbase, unsigned voff, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:1024\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(dst)
                 : "memory");
}
// one 1 KB LDS-DMA piece: lane l's 16 bytes, read from sbase + voff (voff per lane, 32 bit), land at dst + 16 l (dst wave-uniform)
__device__ __forceinline__ void br_glds_piece(const void* sbase, unsigned voff, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(dst)
                 : "memory");
}
// the same with a full 64-bit address per lane (lanes of one piece may read from unrelated places)
__device__ __forceinline__ void br_glds_piece64(const void* vaddr, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(vaddr), "s"(dst)
                 : "memory");
}
// s_waitcnt vmcnt(n) for a value that is a compile-time constant after unrolling (the switch folds away)
__device__ __forceinline__ void br_wait_vm(int n) {
#define BR_W(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        BR_W(0) BR_W(1) BR_W(2) BR_W(3) BR_W(4) BR_W(5) BR_W(6) BR_W(7) BR_W(8) BR_W(9) BR_W(10) BR_W(11) BR_W(12) BR_W(13)
        BR_W(14) BR_W(15) BR_W(16) BR_W(17) BR_W(18) BR_W(19) BR_W(20) BR_W(21) BR_W(22) BR_W(23) BR_W(24) BR_W(25) BR_W(26)
        BR_W(27) BR_W(28) BR_W(29) BR_W(30) BR_W(31) BR_W(32) BR_W(33) BR_W(34) BR_W(35) BR_W(36) BR_W(37) BR_W(38) BR_W(39) BR_W(40)
        BR_W(41) BR_W(42) BR_W(43) BR_W(44) BR_W(45) BR_W(46) BR_W(47) BR_W(48) BR_W(49) BR_W(50) BR_W(51) BR_W(52) BR_W(53) BR_W(54)
        BR_W(55) BR_W(56) BR_W(57) BR_W(58) BR_W(59) BR_W(60) BR_W(61) BR_W(62) BR_W(63)
        default:   // (the counter has six bits; a smaller count is always safe)
            if (n > 63) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            break;
    }
#undef BR_W
}

}  // namespace hgk
