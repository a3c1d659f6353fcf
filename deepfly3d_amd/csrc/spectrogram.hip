// a12 Morlet wavelet spectrogram of a bundle of time series (the model is this project's own specification,
// defined in float64 by tests/spectrogram_oracle.py): S[t, c, i] = |sum_k (a_i[k] + j b_i[k]) x[clamp(t + k), c]|, k = -K_i..K_i.
//
// spectrogram_bank_kernel: one block per row i of the bank writes the row's 2 K_i + 1 tap pairs (a, b) into the caller's workspace,
// after a fixed-order block sum of the Gaussian and of its cosine moment (the normalisation n_i and the admissibility term kappa_i).
//
// spectrogram_kernel: one block per (channel, tile of TILE = 320 consecutive times), four waves.  The block brings
// x[tile -+ Kmax] into LDS once, indices clamped to the series (the edge extension), then walks the rows in chunks of CHUNK = 16.
// Inside a chunk every wave takes its own rows (in snake order, so that the four waves carry nearly equal tap counts); all 64
// lanes of a wave work on the same row and the same tap, so the tap pair is one scalar load for the wave.  A lane owns P = 5
// consecutive times: it keeps a window of five samples in registers, reads ONE new sample from LDS per tap and issues ten
// float64 multiply-adds on it.  P is odd so that the lanes' window reads (a stride of P doubles) fall on 32 different banks.
// Row i runs only its own 2 K_i + 1 taps.  The chunk's amplitudes are collected in LDS as [time][row] and leave the block as runs
// of up to 16 consecutive values per time of the public [T, C, F] layout, float64 or float32 (rounded once).
// No atomics, no scratch.  All float64, default contraction.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int MAX_F = 64;
constexpr int MAX_K = 2048;                    // the cap on a row's half support
constexpr int P = 5;                           // consecutive times per lane
constexpr int WAVES = 4;
constexpr int THREADS = WAVES * df3d::WAVE;    // 256
constexpr int TILE = df3d::WAVE * P;           // 320 times per block
constexpr int CHUNK = 16;                      // rows whose amplitudes are staged together
constexpr int PAD = 16;                        // samples and tap pairs the prefetch may read past a row's end (never used)
constexpr double TWO_PI = 6.283185307179586476925286766559;

struct Bank {
    double f[MAX_F], sigma[MAX_F];
    int K[MAX_F];
    int off[MAX_F];   // the first tap pair of the row, counted in pairs
};

__global__ __launch_bounds__(THREADS) void spectrogram_bank_kernel(Bank bank, double fps, double2* __restrict__ taps) {
    __shared__ double red[2][THREADS];
    const int i = blockIdx.x;
    const double f = bank.f[i], sigma = bank.sigma[i];
    const int K = bank.K[i];
    const double den = 2.0 * sigma * sigma;
    double sg = 0.0, sc = 0.0;
    for (int k = -K + (int)threadIdx.x; k <= K; k += THREADS) {
        const double kk = (double)k;
        const double g = exp(-(kk * kk) / den);
        sg += g;
        sc += g * cos(TWO_PI * f * kk / fps);
    }
    red[0][threadIdx.x] = sg;
    red[1][threadIdx.x] = sc;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    const double norm = 2.0 / red[0][0], kappa = red[1][0] / red[0][0];
    double2* row = taps + bank.off[i];
    for (int k = -K + (int)threadIdx.x; k <= K; k += THREADS) {
        const double kk = (double)k;
        const double g = exp(-(kk * kk) / den);
        const double phi = TWO_PI * f * kk / fps;
        row[k + K] = make_double2(norm * g * (cos(phi) - kappa), -norm * g * sin(phi));
    }
}

// Three groups of P taps from pair `n` on (n a multiple of P).  Tap m multiplies, for the lane's output j, the sample xl[m + j]:
// a group of P taps needs two blocks of P samples.  Sample blocks and tap groups rotate through three buffers each: while a
// group runs, the block and the tap pairs of the NEXT group are already on their way (one LDS read of P samples, one scalar
// load of P pairs, both issued a whole group -- 2 P^2 multiply-adds -- before their first use), so the only wait of a group, at
// its start, finds them landed.  On entry blk[0], blk[1] and tap[0] hold the first group's; on exit they hold the next one's.
// The prefetch runs past the row's end by up to 2 P samples and 2 P pairs, which PAD covers in LDS and in the workspace.
template <bool GUARD>
__device__ __forceinline__ void taps_step(const double2* __restrict__ tp, const double* xl, int n, int ntaps, double (&blk)[3][P],
                                          double2 (&tap)[3][P], double (&A)[P], double (&B)[P]) {
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int m = n + P * h;
        if (GUARD && m >= ntaps) break;
#pragma unroll
        for (int u = 0; u < P; ++u) {
            blk[(h + 2) % 3][u] = xl[m + 2 * P + u];
            tap[(h + 1) % 3][u] = tp[m + P + u];
        }
#pragma unroll
        for (int u = 0; u < P; ++u) {
            if (GUARD && m + u >= ntaps) break;
            const double2 ab = tap[h % 3][u];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const double v = u + j < P ? blk[h % 3][u + j] : blk[(h + 1) % 3][u + j - P];
                A[j] = fma(ab.x, v, A[j]);
                B[j] = fma(ab.y, v, B[j]);
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void spectrogram_kernel(const double* __restrict__ x, long long T, int C, int F, int Kmax, Bank bank,
                                                              const double2* __restrict__ taps, void* __restrict__ out, int f32) {
    extern __shared__ double lds[];
    const int nx = TILE + 2 * Kmax;
    double* xs = lds;            // xs[j] = x[clamp(t0 - Kmax + j)], j < nx
    double* stage = lds + nx + PAD;   // [TILE][CHUNK]
    const int c = (int)(blockIdx.x % (unsigned)C);
    const long long t0 = (long long)(blockIdx.x / (unsigned)C) * TILE;
    const double* xc = x + (long long)c * T;
    for (int j = threadIdx.x; j < nx; j += THREADS) {
        long long t = t0 - Kmax + j;
        t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
        xs[j] = xc[t];
    }
    __syncthreads();
    const int lane = threadIdx.x & (df3d::WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / df3d::WAVE);
    const long long left = T - t0;
    const int live = (int)(left < TILE ? left : TILE);
    for (int i0 = 0; i0 < F; i0 += CHUNK) {
        const int rows = F - i0 < CHUNK ? F - i0 : CHUNK;
#pragma unroll 1
        for (int s = 0; s < CHUNK / WAVES; ++s) {
            const int r = (s & 1) ? WAVES * s + WAVES - 1 - wave : WAVES * s + wave;   // 0..3, 7..4, 8..11, 15..12
            if (r >= rows) continue;
            const int K = bank.K[i0 + r], ntaps = 2 * K + 1;
            const double2* tp = taps + bank.off[i0 + r];
            const double* xl = xs + (Kmax - K + P * lane);   // the lane's first time, tap -K
            double A[P], B[P], blk[3][P];
            double2 tap[3][P];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                A[j] = B[j] = 0.0;
                blk[0][j] = xl[j];
                blk[1][j] = xl[P + j];
                tap[0][j] = tp[j];
            }
            int n = 0;
#pragma unroll 1
            for (; n + 3 * P <= ntaps; n += 3 * P) taps_step<false>(tp, xl, n, ntaps, blk, tap, A, B);
            taps_step<true>(tp, xl, n, ntaps, blk, tap, A, B);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const bool ok = isfinite(A[j]) && isfinite(B[j]);
                stage[(P * lane + j) * CHUNK + r] = ok ? sqrt(A[j] * A[j] + B[j] * B[j]) : __builtin_nan("");
            }
        }
        __syncthreads();
        const int count = live * rows;
        for (int e = threadIdx.x; e < count; e += THREADS) {
            const int tl = e / rows, r = e - tl * rows;
            const double v = stage[tl * CHUNK + r];
            const long long at = ((t0 + tl) * C + c) * F + i0 + r;
            if (f32) {
                static_cast<float*>(out)[at] = (float)v;
            } else {
                static_cast<double*>(out)[at] = v;
            }
        }
        __syncthreads();
    }
}

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, long long na, const void* b, long long nb) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
}

struct Plan {
    Bank bank;
    int Kmax;
    long long pairs;   // tap pairs of the whole bank
};

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// the bank's geometry from its parameters; DF3D_EINVAL with the message set where they are refused
int make_plan(const char* fn, const double* freqs_host, int F, double fps, double omega0, double radius, Plan& plan) {
    if (F < 1 || F > MAX_F) {
        df3d::set_error("%s: F must be in [1, %d] (it is %d)", fn, MAX_F, F);
        return DF3D_EINVAL;
    }
    if (!positive(fps) || !positive(omega0) || !positive(radius)) {
        df3d::set_error("%s: %s must be finite and > 0", fn, !positive(fps) ? "fps" : !positive(omega0) ? "omega0" : "radius");
        return DF3D_EINVAL;
    }
    if (!freqs_host) {
        df3d::set_error("%s: null pointer: freqs", fn);
        return DF3D_EINVAL;
    }
    if (!positive(freqs_host[0])) {
        df3d::set_error("%s: f_min (freqs[0]) must be finite and > 0", fn);
        return DF3D_EINVAL;
    }
    for (int i = 1; i < F; ++i) {
        if (!(freqs_host[i] >= freqs_host[i - 1])) {
            df3d::set_error("%s: the frequencies must ascend from f_min to f_max: f_max < f_min, or freqs[%d] < freqs[%d]", fn, i, i - 1);
            return DF3D_EINVAL;
        }
    }
    if (!(freqs_host[F - 1] <= fps / 2.0)) {
        df3d::set_error("%s: f_max (%g) must be at most fps/2 (%g)", fn, freqs_host[F - 1], fps / 2.0);
        return DF3D_EINVAL;
    }
    memset(&plan, 0, sizeof(plan));
    for (int i = 0; i < F; ++i) {
        const double f = freqs_host[i];
        const double sigma = omega0 * fps / (TWO_PI * f);
        const double k = std::ceil(radius * sigma);
        if (!(k <= (double)MAX_K)) {
            df3d::set_error("%s: the support K_0 = ceil(radius * omega0 * fps / (2 pi f_min)) = %.0f samples is above the kernel's cap of %d: "
                            "the smallest f_min that fits is %.9g Hz",
                            fn, k, MAX_K, radius * omega0 * fps / (TWO_PI * MAX_K));
            return DF3D_EINVAL;
        }
        plan.bank.f[i] = f;
        plan.bank.sigma[i] = sigma;
        plan.bank.K[i] = (int)k;
        plan.bank.off[i] = (int)plan.pairs;
        plan.pairs += 2 * (long long)k + 1;
        if ((int)k > plan.Kmax) plan.Kmax = (int)k;
    }
    return DF3D_OK;
}

long long work_bytes(const Plan& plan) { return (plan.pairs + PAD) * (long long)sizeof(double2); }

}  // namespace

extern "C" int df3d_spectrogram_tile(void) { return TILE; }

extern "C" long long df3d_spectrogram_work_bytes(const double* freqs_host, int F, double fps, double omega0, double radius) {
    Plan plan;
    if (make_plan(__func__, freqs_host, F, fps, omega0, radius, plan) != DF3D_OK) return 0;
    return work_bytes(plan);
}

extern "C" int df3d_spectrogram_bank(const double* freqs_host, int F, double fps, double omega0, double radius, void* work_dev,
                                     long long work_len_bytes, void* stream) {
    Plan plan;
    if (const int rc = make_plan(__func__, freqs_host, F, fps, omega0, radius, plan)) return rc;
    DF3D_CHECK_ARG(work_dev, "null pointer: work");
    DF3D_CHECK_ARG(((uintptr_t)work_dev & 15) == 0, "work must be 16-byte aligned");
    DF3D_CHECK_ARG(work_len_bytes >= work_bytes(plan), "work buffer too small (df3d_spectrogram_work_bytes)");
    hipLaunchKernelGGL(spectrogram_bank_kernel, dim3((unsigned)F), dim3(THREADS), 0, df3d::as_stream(stream), plan.bank, fps,
                       static_cast<double2*>(work_dev));
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_spectrogram(const double* x_dev, long long T, int C, const double* freqs_host, int F, double fps, double omega0,
                                double radius, const void* work_dev, long long work_len_bytes, void* out_dev, int out_f32, void* stream) {
    DF3D_CHECK_ARG(T >= 0, "T must be >= 0");
    DF3D_CHECK_ARG(C >= 1, "C must be >= 1");
    Plan plan;
    if (const int rc = make_plan(__func__, freqs_host, F, fps, omega0, radius, plan)) return rc;
    DF3D_CHECK_ARG(out_f32 == 0 || out_f32 == 1, "out_f32 must be 0 (float64 output) or 1 (float32 output)");
    const long long tiles = (T + TILE - 1) / TILE;
    DF3D_CHECK_ARG(tiles * C <= 0x7fffffffLL && T <= (1LL << 62) / C / F / 8, "T * C is too large (one grid dimension holds ceil(T / 320) * C blocks)");
    if (T == 0) return DF3D_OK;
    const int esize = out_f32 ? 4 : 8;
    DF3D_CHECK_ARG(x_dev && work_dev && out_dev, "null pointer (x, work or out)");
    DF3D_CHECK_ARG(((uintptr_t)x_dev & 7) == 0 && ((uintptr_t)out_dev & (esize - 1)) == 0, "x must be 8-byte aligned and out aligned to its element");
    DF3D_CHECK_ARG(((uintptr_t)work_dev & 15) == 0, "work must be 16-byte aligned");
    DF3D_CHECK_ARG(work_len_bytes >= work_bytes(plan), "work buffer too small (df3d_spectrogram_work_bytes)");
    const long long nx = T * C * 8, no = T * C * F * esize, nw = work_bytes(plan);
    DF3D_CHECK_ARG(!overlap(out_dev, no, x_dev, nx), "out must not overlap x");
    DF3D_CHECK_ARG(!overlap(work_dev, nw, x_dev, nx) && !overlap(work_dev, nw, out_dev, no), "work must not overlap x or out");
    const size_t lds = sizeof(double) * (size_t)(TILE + 2 * plan.Kmax + PAD + TILE * CHUNK);   // at most 76 416 bytes
    // the attribute belongs to the CURRENT device, and a process may drive several: set on every launch that needs it
    if (lds > 64 * 1024)
        DF3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(spectrogram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(spectrogram_kernel, dim3((unsigned)(tiles * C)), dim3(THREADS), lds, df3d::as_stream(stream), x_dev, T, C, F, plan.Kmax,
                       plan.bank, static_cast<const double2*>(work_dev), out_dev, out_f32);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
