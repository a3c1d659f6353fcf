// The arg-max kernel of argmax.hip (plain) and subpixel.hip (SUBPIXEL: the winner refined from its 3 x 3 neighbourhood, DESIGN.md
// section 12).  The scan and the wave reduction are shared, so both entries pick the same cell, the same confidence and count
// non-finite planes the same way.
#pragma once
#include "subpixel_dev.h"

namespace df3d {

struct Best {
    float v;
    int i;
};

__device__ __forceinline__ Best better(Best a, Best b) {
    // NaN never wins (comparisons with NaN are false); -inf planes resolve to index 0 via the seed
    bool take_b = (b.v > a.v) || (b.v == a.v && b.i < a.i);
    return take_b ? b : a;
}

template <bool SUBPIXEL>
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ hm, int planes, int hw, int w,
                                                     float inv_h, float inv_w, float* __restrict__ pts,
                                                     float* __restrict__ conf, int* __restrict__ nonfinite_planes) {
    const int lane = threadIdx.x & 63;
    const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const float4* src = reinterpret_cast<const float4*>(hm + (size_t)plane * hw);
    const int nvec = hw >> 2;

    Best best{-__builtin_inff(), 0x7fffffff};
    unsigned mag = 0;   // max of |x| as an integer: >= 0x7f800000 <=> an infinity or a NaN was among the values (the overflow guard of the 16-bit / f32s engines)
    auto seen = [&](const float4& q) {
        mag = max(max(mag, __float_as_uint(q.x) & 0x7fffffffu), max(__float_as_uint(q.y) & 0x7fffffffu, max(__float_as_uint(q.z) & 0x7fffffffu, __float_as_uint(q.w) & 0x7fffffffu)));
    };
    int i = lane;
    // 4 independent 16-B loads in flight per lane
    for (; i + 192 < nvec; i += 256) {
        float4 a = src[i], b = src[i + 64], c = src[i + 128], d = src[i + 192];
        const float4 q[4] = {a, b, c, d};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            seen(q[u]);
            const int base = (i + 64 * u) * 4;
            if (q[u].x > best.v) best = Best{q[u].x, base};
            if (q[u].y > best.v) best = Best{q[u].y, base + 1};
            if (q[u].z > best.v) best = Best{q[u].z, base + 2};
            if (q[u].w > best.v) best = Best{q[u].w, base + 3};
        }
    }
    for (; i < nvec; i += 64) {
        float4 a = src[i];
        seen(a);
        const int base = i * 4;
        if (a.x > best.v) best = Best{a.x, base};
        if (a.y > best.v) best = Best{a.y, base + 1};
        if (a.z > best.v) best = Best{a.z, base + 2};
        if (a.w > best.v) best = Best{a.w, base + 3};
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Best o;
        o.v = __shfl_xor(best.v, off, 64);
        o.i = __shfl_xor(best.i, off, 64);
        best = better(best, o);
        mag = max(mag, (unsigned)__shfl_xor((int)mag, off, 64));
    }
    if (lane == 0) {
        if (nonfinite_planes && mag >= 0x7f800000u) atomicAdd(nonfinite_planes, 1);
        int idx = best.i == 0x7fffffff ? 0 : best.i;
        float v = best.i == 0x7fffffff ? hm[(size_t)plane * hw] : best.v;
        if constexpr (SUBPIXEL) {
            // the nine values round the winner were read a moment ago by this wave: at most nine cache lines, no second pass
            const float* p = hm + (size_t)plane * hw;
            subpixel_point([&](int r, int c) { return p[r * w + c]; }, idx / w, idx % w, hw / w, w, (double)inv_h, (double)inv_w,
                           &pts[2 * (size_t)plane + 0], &pts[2 * (size_t)plane + 1]);
        } else {
            pts[2 * (size_t)plane + 0] = (float)(idx / w) * inv_h;
            pts[2 * (size_t)plane + 1] = (float)(idx % w) * inv_w;
        }
        conf[plane] = v;
    }
}


}  // namespace df3d
