// The single-convolution kernel of the stacked-hourglass engine (a2).  NHWC activations, gfx950 MFMA.  (The other device families: hg_stem.h,
// hg_pool.h, hg_bt_*.h, hg_l1_*.h, hg_c1_*.h, hg_head.h; all on hg_types.h.)
//
//   conv_mfma_kernel<T, TAPS, BN, RB>
//       1x1 (TAPS=1) and 3x3/pad 1 (TAPS=9) convolutions as an implicit GEMM
//           out[m, n] = sum_{tap, c} act(in[pixel(m) + tap, c]) * W[tap][n][c]  (+ bias, + residual, ReLU)
//       with m = (view, y, x) flattened.  Workgroup tile 128 pixels x BN channels, 4 wavefronts, each owning
//       32x32 MFMA tiles (v_mfma_f32_32x32x2_f32 for T=float: exact f32 FMA chains at the 157 TF rate;
//       v_mfma_f32_32x32x16_bf16 / _f16 for the 16-bit engines, T = __hip_bfloat16 / _Float16: see Lp<T>).  Per K-step both operands are staged global -> registers -> LDS
//       as RB-byte row segments (16-byte chunks), double-buffered with one barrier per step; the global loads
//       for step s+1 are issued before the MFMAs of step s.  Rows are padded by 16 bytes in LDS, which makes
//       the 16-byte ds_read of a 32-row fragment conflict-free (row pitch 80 B / 144 B: see DESIGN.md).
//       A 16-byte fragment holds 4 (f32) or 8 (bf16) consecutive K values of one row; lanes 0-31 take the
//       even 16-byte chunk and lanes 32-63 the odd one, which permutes K inside the step identically for
//       both operands (the sum over K is unchanged).
//       Fusions: eval-mode BN + ReLU of the *input* (pre-activation bottlenecks) while staging; bias, residual
//       add and ReLU in the epilogue; optional NCHW plane output for the final heat-maps.
#pragma once
#include "hg_types.h"

namespace hgk {

struct ConvArgs {
    const void* in;
    void* out;          // NHWC [M, out_pitch] (may be null when only the NCHW output is wanted)
    const void* res;    // NHWC residual [M, res_pitch] or null
    float* out_nchw;    // float32 planes [views, cout_real, H*W] or null
    const void* w;      // [TAPS][cout][cin]  (T)
    const float* bias;  // [cout] f32
    const float* scale; // [cin] f32 or null: input BN as x*scale+shift then ReLU
    const float* shift;
    long long M;        // views * H * W
    int H, W;
    int cin, cout;      // padded: cin multiple of RB/sizeof(T), cout multiple of BN
    int in_pitch, out_pitch, res_pitch;
    int relu;
    int cout_real;
};

// Tile geometry for a given BN
template <int BN>
struct Geo;
template <>
struct Geo<128> { static constexpr int WM = 2, WN = 2, TM = 2, TN = 2; };
template <>
struct Geo<64> { static constexpr int WM = 2, WN = 2, TM = 2, TN = 1; };
template <>
struct Geo<32> { static constexpr int WM = 4, WN = 1, TM = 1, TN = 1; };

constexpr int BM = 128;

template <typename T, int TAPS, int BN, int RB>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs p) {
    using G = Geo<BN>;
    constexpr int PITCH = RB + 16;                 // LDS row pitch in bytes
    constexpr int CPR = RB / 16;                   // 16-byte chunks per row per step
    constexpr int ROWS_PER_PASS = 256 / CPR;       // rows covered by one pass of the 256 threads
    constexpr int A_PASSES = BM / ROWS_PER_PASS;
    constexpr int B_PASSES = (BN + ROWS_PER_PASS - 1) / ROWS_PER_PASS;
    constexpr int KE = RB / Elem<T>::BYTES;        // K elements per step
    constexpr int A_BYTES = BM * PITCH, B_BYTES = BN * PITCH;
    static_assert(BN % 32 == 0 && A_PASSES >= 1, "tile");

    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;  // one pipeline stage: A tile then B tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / G::WN, wn = wave % G::WN;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    // ---- staging assignment: thread -> (row, 16-byte chunk) ------------------------------------------
    const int chunk = tid % CPR;
    const int srow = tid / CPR;
    const unsigned char* a_ptr[A_PASSES];  // pointer to in[pixel][0] (bytes) for each staged row
    int a_yx[A_PASSES];                    // (y << 16) | x, or -1 when the row is beyond M
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
        const long long m = m0 + srow + i * ROWS_PER_PASS;
        if (m < p.M) {
            const int hw = p.H * p.W;
            const int pix = (int)(m % hw);
            a_yx[i] = ((pix / p.W) << 16) | (pix % p.W);
            a_ptr[i] = reinterpret_cast<const unsigned char*>(p.in) + (size_t)m * p.in_pitch * Elem<T>::BYTES;
        } else {
            a_yx[i] = -1;
            a_ptr[i] = reinterpret_cast<const unsigned char*>(p.in);
        }
    }
    const int ksteps_per_tap = p.cin / KE;
    const int nsteps = TAPS * ksteps_per_tap;

    u32x4 ra[A_PASSES], rb[B_PASSES];
    bool ra_ok[A_PASSES];
    PreactCoef<T> coef;

    auto load_step = [&](int s) {
        const int tap = TAPS == 1 ? 0 : s / ksteps_per_tap;
        const int kc = TAPS == 1 ? s : s - tap * ksteps_per_tap;
        const int c0 = kc * KE + chunk * Elem<T>::PER16;  // first channel of this thread's chunk
        int dy = 0, dx = 0;
        if (TAPS == 9) {
            dy = tap / 3 - 1;
            dx = tap % 3 - 1;
        }
        const long long tap_off = ((long long)dy * p.W + dx) * p.in_pitch * Elem<T>::BYTES;
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            bool ok = a_yx[i] >= 0;
            if (TAPS == 9 && ok) {
                const int y = (a_yx[i] >> 16) + dy, x = (a_yx[i] & 0xffff) + dx;
                ok = (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
            }
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *reinterpret_cast<const u32x4*>(a_ptr[i] + tap_off + (size_t)c0 * Elem<T>::BYTES);
            ra[i] = v;
            ra_ok[i] = ok;
        }
        if (TAPS == 1 && p.scale) coef.load(p.scale, p.shift, c0);
        const unsigned char* wbase = reinterpret_cast<const unsigned char*>(p.w) +
                                     ((size_t)tap * p.cout * p.cin + (size_t)c0) * Elem<T>::BYTES;
#pragma unroll
        for (int i = 0; i < B_PASSES; ++i) {
            const int n = srow + i * ROWS_PER_PASS;
            if (BN % ROWS_PER_PASS == 0 || n < BN)
                rb[i] = *reinterpret_cast<const u32x4*>(wbase + (size_t)(n0 + n) * p.cin * Elem<T>::BYTES);
        }
    };
    auto store_step = [&](int buf) {
        unsigned char* const sa = smem + buf * STAGE_BYTES;
        unsigned char* const sb = sa + A_BYTES;
        // the input BN + ReLU is applied here, AFTER the MFMAs of the current step, so the global loads issued by
        // load_step() stay in flight across the whole compute phase
        if (TAPS == 1 && p.scale) {
#pragma unroll
            for (int i = 0; i < A_PASSES; ++i)
                if (ra_ok[i]) ra[i] = preact_apply<T>(ra[i], coef);
        }
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i)
            *reinterpret_cast<u32x4*>(sa + (srow + i * ROWS_PER_PASS) * PITCH + chunk * 16) = ra[i];
#pragma unroll
        for (int i = 0; i < B_PASSES; ++i) {
            const int n = srow + i * ROWS_PER_PASS;
            if (BN % ROWS_PER_PASS == 0 || n < BN) *reinterpret_cast<u32x4*>(sb + n * PITCH + chunk * 16) = rb[i];
        }
    };

    f32x16 acc[G::TM][G::TN];
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
        for (int j = 0; j < G::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // fragment read offsets (bytes) inside a tile
    const int frag_row = lane & 31;
    const int frag_half = (lane >> 5) * 16;
    const int a_off = (wm * (G::TM * 32) + frag_row) * PITCH + frag_half;
    const int b_off = (wn * (G::TN * 32) + frag_row) * PITCH + frag_half;

    load_step(0);
    store_step(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        const unsigned char* const sa = smem + buf * STAGE_BYTES;
        const unsigned char* const sb = sa + A_BYTES;
        if (s + 1 < nsteps) load_step(s + 1);
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch loads ABOVE the MFMA block (hipcc sinks them otherwise)
#pragma unroll
        for (int j = 0; j < RB / 32; j += 2) {   // fragment pairs (j, j + 1) = one 64-byte step of K (float32: 16 values) per lane pair, see mfma_pair
            XPair<T> af[G::TM];
            u32x4 bf[G::TN][2];
#pragma unroll
            for (int i = 0; i < G::TM; ++i)
                af[i] = make_xpair<T>(*reinterpret_cast<const u32x4*>(sa + a_off + i * 32 * PITCH + j * 32), *reinterpret_cast<const u32x4*>(sa + a_off + i * 32 * PITCH + (j + 1) * 32));
#pragma unroll
            for (int i = 0; i < G::TN; ++i)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) bf[i][jj] = *reinterpret_cast<const u32x4*>(sb + b_off + i * 32 * PITCH + (j + jj) * 32);
#pragma unroll
            for (int i = 0; i < G::TM; ++i)
#pragma unroll
                for (int k = 0; k < G::TN; ++k) mfma_pair<T, false>(bf[k][0], bf[k][1], af[i], acc[i][k]);
        }
        if (s + 1 < nsteps) store_step(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue ------------------------------------------------------------------------------------
    // C layout of the 32x32 MFMA: column (channel) = lane & 31, row (pixel) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int hw = p.H * p.W;
#pragma unroll
    for (int j = 0; j < G::TN; ++j) {
        const int n = n0 + wn * (G::TN * 32) + j * 32 + (lane & 31);
        const float bias = p.bias[n];
#pragma unroll
        for (int i = 0; i < G::TM; ++i) {
            const long long mbase = m0 + wm * (G::TM * 32) + i * 32 + 4 * (lane >> 5);
            // all 16 residual loads of the tile are issued before the first store (loads may not pass stores
            // to possibly aliasing memory, so interleaving them would serialise 16 round trips)
            float resv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = mbase + (r & 3) + 8 * (r >> 2);
                resv[r] = 0.0f;
                if (p.res && m < p.M) {
                    if constexpr (sizeof(T) == 4)
                        resv[r] = reinterpret_cast<const float*>(p.res)[(size_t)m * p.res_pitch + n];
                    else
                        resv[r] = Lp<T>::to_f32(reinterpret_cast<const unsigned short*>(p.res)[(size_t)m * p.res_pitch + n]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = mbase + (r & 3) + 8 * (r >> 2);
                float v = acc[i][j][r] + bias;
                if (m < p.M) {
                    v += resv[r];
                    if (p.relu) v = fmaxf(v, 0.0f);
                    if (p.out) {
                        if constexpr (sizeof(T) == 4)
                            reinterpret_cast<float*>(p.out)[(size_t)m * p.out_pitch + n] = v;
                        else
                            reinterpret_cast<unsigned short*>(p.out)[(size_t)m * p.out_pitch + n] = Lp<T>::from_f32(v);
                    }
                }
                acc[i][j][r] = v;
            }
            if (p.out_nchw && n < p.cout_real) {
                // 4 consecutive registers = 4 consecutive pixels of one plane
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long long m = mbase + 8 * q;
                    if (m + 3 < p.M) {
                        const long long view = m / hw;
                        const int pix = (int)(m - view * hw);
                        f32x4 o = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                        *reinterpret_cast<f32x4*>(p.out_nchw + ((size_t)view * p.cout_real + n) * hw + pix) = o;
                    }
                }
            }
        }
    }
}

}  // namespace hgk
