// The peaks kernel of pictorial.hip (plain) and subpixel.hip (SUBPIXEL: every peak refined from its 3 x 3 neighbourhood in LDS,
// DESIGN.md section 12).  Detection, order, count and values are shared code, so they are the same in both.
#pragma once
#include <climits>

#include "subpixel_dev.h"

namespace df3d {

constexpr int KMAX = 16;    // peaks per plane
constexpr int PEAK_BLOCK = 64;
constexpr int MASK_WORDS = 4;   // peak flags of a lane's cells: 128 bits

template <bool SUBPIXEL>
__global__ __launch_bounds__(PEAK_BLOCK) void peaks_kernel(const float* __restrict__ hm, int hw, int w, int wshift, int k,
                                                           float inv_h, float inv_w, int* __restrict__ count,
                                                           float* __restrict__ pts, float* __restrict__ vals) {
    extern __shared__ float s[];
    const int lane = threadIdx.x;
    const long long plane = blockIdx.x;
    const float4* src = reinterpret_cast<const float4*>(hm + plane * hw);
    float4* dst = reinterpret_cast<float4*>(s);
    const int nvec = hw >> 2;
    int i = lane;
    for (; i + 7 * 64 < nvec; i += 8 * 64) {   // 8 independent 16-byte loads in flight per lane
        float4 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = src[i + 64 * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[i + 64 * u] = q[u];
    }
    for (; i < nvec; i += 64) dst[i] = src[i];
    __syncthreads();

    // phase 1: which of this lane's cells are peaks (bit u of mask[u / 32] <=> cell lane + 64 u).  fmaxf ignores NaN operands, so a
    // non-finite neighbour (+inf read as NaN) drops out of the neighbourhood maxima; a non-finite cell fails both comparisons
    const int h = hw >> wshift;
    const int nit = hw >> 6;
    unsigned mask[MASK_WORDS] = {0u, 0u, 0u, 0u};   // up to 128 cells per lane: h * w <= 8192
    auto cell = [&](int r, int c) -> float {
        const float q = s[(r << wshift) + c];
        return isfinite(q) ? q : __builtin_nanf("");
    };
#pragma unroll
    for (int wd = 0; wd < MASK_WORDS; ++wd)
    for (int b = 0; b < 32; ++b) {
        const int u = 32 * wd + b;
        if (u >= nit) break;
        const int p = lane + 64 * u;
        const int r = p >> wshift, c = p & (w - 1);
        const float v = cell(r, c);
        float mb = -__builtin_inff(), ma = -__builtin_inff();   // maxima of the neighbours before / after p in row-major order
        const bool up = r > 0, dn = r + 1 < h, lf = c > 0, rt = c + 1 < w;
        if (up) {
            mb = fmaxf(mb, cell(r - 1, c));
            if (lf) mb = fmaxf(mb, cell(r - 1, c - 1));
            if (rt) mb = fmaxf(mb, cell(r - 1, c + 1));
        }
        if (lf) mb = fmaxf(mb, cell(r, c - 1));
        if (rt) ma = fmaxf(ma, cell(r, c + 1));
        if (dn) {
            ma = fmaxf(ma, cell(r + 1, c));
            if (lf) ma = fmaxf(ma, cell(r + 1, c - 1));
            if (rt) ma = fmaxf(ma, cell(r + 1, c + 1));
        }
        if (v > mb && v >= ma) mask[wd] |= 1u << b;
    }

    // phase 2: the lane's peaks, in increasing flat index, into a sorted register top-16 (value descending, then index ascending:
    // an equal value arriving later has the larger index and goes behind)
    float tv[KMAX];
    int ti[KMAX];
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
        tv[u] = -__builtin_inff();
        ti[u] = INT_MAX;
    }
#pragma unroll
    for (int wd = 0; wd < MASK_WORDS; ++wd) {
        unsigned bits = mask[wd];
        while (bits) {
            const int u = 32 * wd + __builtin_ctz(bits);
            bits &= bits - 1;
            const int p = lane + 64 * u;
            const float v = s[p];
            if (!(v > tv[KMAX - 1])) continue;
#pragma unroll
            for (int x = KMAX - 1; x > 0; --x) {
                const bool upx = v > tv[x - 1];
                const bool here = !upx && v > tv[x];
                tv[x] = upx ? tv[x - 1] : (here ? v : tv[x]);
                ti[x] = upx ? ti[x - 1] : (here ? p : ti[x]);
            }
            if (v > tv[0]) {
                tv[0] = v;
                ti[0] = p;
            }
        }
    }
    // merge: K rounds of a wave-wide max of every lane's head; the winning lane pops it
    int n = 0;
    [[maybe_unused]] int mine = 0;
    for (int r = 0; r < k; ++r) {
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi == INT_MAX) break;   // wave-uniform: no lane holds another peak
        if (ti[0] == bi) {
#pragma unroll
            for (int u = 0; u < KMAX - 1; ++u) {
                tv[u] = tv[u + 1];
                ti[u] = ti[u + 1];
            }
            tv[KMAX - 1] = -__builtin_inff();
            ti[KMAX - 1] = INT_MAX;
        }
        if constexpr (SUBPIXEL) {
            if (lane == r) mine = bi;   // lane r refines peak r after the merge: the K peaks in parallel
            if (lane == 0) vals[plane * k + r] = bv;
        } else if (lane == 0) {
            // the normalised convention (and arithmetic) of argmax_kernel
            pts[(plane * k + r) * 2 + 0] = (float)(bi >> wshift) * inv_h;
            pts[(plane * k + r) * 2 + 1] = (float)(bi & (w - 1)) * inv_w;
            vals[plane * k + r] = bv;
        }
        n = r + 1;
    }
    if (lane == 0) count[plane] = n;
    if constexpr (SUBPIXEL) {
        if (lane < n)   // the neighbours come from the plane in LDS; peak 0 is then the refined arg-max point bit for bit
            subpixel_point([&](int rr, int cc) { return s[(rr << wshift) + cc]; }, mine >> wshift, mine & (w - 1), h, w, (double)inv_h,
                           (double)inv_w, &pts[(plane * k + lane) * 2 + 0], &pts[(plane * k + lane) * 2 + 1]);
    }
    for (int r = n + lane; r < k; r += 64) {
        pts[(plane * k + r) * 2 + 0] = 0.0f;
        pts[(plane * k + r) * 2 + 1] = 0.0f;
        vals[plane * k + r] = 0.0f;
    }
}

}  // namespace df3d
