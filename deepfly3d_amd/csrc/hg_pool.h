// The hourglass' bandwidth-bound passes, one thread per 16-byte channel chunk: 2x2 max-pool, nearest-upsample + add, the parity export
// and the float32 -> 16-bit weight conversion, with the chunk helpers (max_chunk, add_chunk) the fused bottleneck epilogues share.
#pragma once
#include "hg_types.h"

namespace hgk {

// -----------------------------------------------------------------------------------------------------
// 2x2 max-pool and nearest-upsample + add: one thread per 16-byte channel chunk
// -----------------------------------------------------------------------------------------------------
// bf16 as an ORDERED 16-bit integer and back (the map is its own inverse): a negative float's magnitude bits are flipped, so
// that signed integer comparison orders the keys like the floats (-0 just below +0).  Lets max() of packed bf16 run as one
// v_pk_max_i16 per two values instead of unpack + three v_max_f32 (the NaN-quieting hipcc adds) + repack.
typedef short hg_i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf16x2_key(unsigned v) {
    const hg_i16x2 x = __builtin_bit_cast(hg_i16x2, v);
    const hg_i16x2 m = (x >> 15) & (short)0x7fff;
    return __builtin_bit_cast(unsigned, x ^ m);
}
__device__ __forceinline__ unsigned bf16x2_key_max(unsigned ka, unsigned kb) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(hg_i16x2, ka), __builtin_bit_cast(hg_i16x2, kb)));
}
__device__ __forceinline__ u32x4 bf16_key_chunk(u32x4 v) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = bf16x2_key(v[i]);
    return o;
}
__device__ __forceinline__ u32x4 bf16_key_max_chunk(u32x4 a, u32x4 b) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = bf16x2_key_max(a[i], b[i]);
    return o;
}

// element-wise maximum of one 16-byte chunk (finite values; of +0 and -0 the bf16 form returns +0)
template <typename T>
__device__ __forceinline__ u32x4 max_chunk(u32x4 a, u32x4 b) {
    if constexpr (sizeof(T) == 4) {
        f32x4 x = __builtin_bit_cast(f32x4, a), y = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = fmaxf(x[i], y[i]);
        return __builtin_bit_cast(u32x4, x);
    } else if constexpr (std::is_same<T, _Float16>::value) {
        // IEEE half has a packed maximum of its own: one instruction per two values (the ordered-integer detour of the bf16 form
        // costs seven).  Inline assembly on purpose: the builtin brings a NaN-quieting v_pk_max_f16 per operand; pooled values only
        // ever go to stores and lane shuffles, never straight into an MFMA (see br_relu_pk on that hazard)
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) asm("v_pk_max_f16 %0, %1, %2" : "=v"(o[i]) : "v"(a[i]), "v"(b[i]));
        return o;
    } else {
        return bf16_key_chunk(bf16_key_max_chunk(bf16_key_chunk(a), bf16_key_chunk(b)));
    }
}
template <typename T>
__device__ __forceinline__ u32x4 add_chunk(u32x4 a, u32x4 b) {
    if constexpr (sizeof(T) == 4) {
        f32x4 x = __builtin_bit_cast(f32x4, a), y = __builtin_bit_cast(f32x4, b);
        x += y;
        return __builtin_bit_cast(u32x4, x);
    } else {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float al = Lp<T>::to_f32((unsigned short)(a[i] & 0xffffu)), ah = Lp<T>::to_f32((unsigned short)(a[i] >> 16));
            const float bl = Lp<T>::to_f32((unsigned short)(b[i] & 0xffffu)), bh = Lp<T>::to_f32((unsigned short)(b[i] >> 16));
            o[i] = Lp<T>::pack2(al + bl, ah + bh);
        }
        return o;
    }
}

// in [V, H, W, C] -> out [V, H/2, W/2, C];  chunks = C * sizeof(T) / 16 per pixel
template <typename T>
__global__ __launch_bounds__(256) void pool2_kernel(const u32x4* __restrict__ in, u32x4* __restrict__ out, long long total,
                                                    int OH, int OW, int chunks) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % chunks);
    long long pidx = idx / chunks;
    const int ox = (int)(pidx % OW);
    pidx /= OW;
    const int oy = (int)(pidx % OH);
    const long long v = pidx / OH;
    const int W = OW * 2;
    const size_t base = (((size_t)v * OH * 2 + 2 * oy) * W + 2 * ox) * chunks + ch;
    const u32x4 a = in[base], b = in[base + chunks], c = in[base + (size_t)W * chunks], d = in[base + (size_t)W * chunks + chunks];
    out[idx] = max_chunk<T>(max_chunk<T>(a, b), max_chunk<T>(c, d));
}

// out[v, y, x, :] = a[v, y, x, :] + b[v, y/2, x/2, :]   (out may alias a)
template <typename T>
__global__ __launch_bounds__(256) void upadd_kernel(const u32x4* a, const u32x4* __restrict__ b, u32x4* out, long long total,
                                                    int H, int W, int chunks) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % chunks);
    long long pidx = idx / chunks;
    const int x = (int)(pidx % W);
    pidx /= W;
    const int y = (int)(pidx % H);
    const long long v = pidx / H;
    const size_t bidx = (((size_t)v * (H / 2) + (y >> 1)) * (W / 2) + (x >> 1)) * chunks + ch;
    out[idx] = add_chunk<T>(a[idx], b[bidx]);
}

// debug / parity export: NHWC with channel pitch -> dense float32 NHWC with c channels
template <typename T>
__global__ __launch_bounds__(256) void export_kernel(const void* __restrict__ in, float* __restrict__ out, long long pixels,
                                                     int c, int pitch) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= pixels * c) return;
    const long long pix = idx / c;
    const int ch = (int)(idx % c);
    if constexpr (sizeof(T) == 4)
        out[idx] = reinterpret_cast<const float*>(in)[(size_t)pix * pitch + ch];
    else
        out[idx] = Lp<T>::to_f32(reinterpret_cast<const unsigned short*>(in)[(size_t)pix * pitch + ch]);
}

// weights f32 -> 16-bit storage format (round to nearest even)
template <typename T>
__global__ __launch_bounds__(256) void f32_to_lp_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = Lp<T>::from_f32(in[i]);
}

}  // namespace hgk
