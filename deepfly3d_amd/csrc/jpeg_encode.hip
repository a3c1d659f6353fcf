// Baseline JPEG encoder on the device: n RGB frames -> n entropy-coded scans, byte-equal to libjpeg's
// (Pillow's) for 4:2:0, the Annex K Huffman tables and no restart markers.  The Motion-JPEG video path's other half of csrc/jpeg.hip.
//
// Seven launches per batch, all on the caller's stream, all integer arithmetic:
//   blocks   one workgroup per run of four MCUs (a 64 x 16 pixel strip): RGB -> LDS (dwords where 3 W is a multiple of 4), colour
//            conversion, h2v2 downsampling, both "islow" DCT passes in LDS, quantisation, int16 coefficients in zigzag order with the
//            dummy blocks already filled (their source block is always in the same MCU)
//   bits     one wave per block: lane k holds coefficient k, the non-zero mask is one ballot, every lane knows its symbol's length;
//            bits per block and per group of 32 blocks
//   offsets  one workgroup per frame: exclusive scan of the group totals (64-bit bit offsets), the frame's unstuffed length; clears
//            the words two groups share
//   emit     one workgroup per group: every lane composes its symbol (up to 59 bits) into an LDS bit buffer, whole words are stored;
//            a word shared with a neighbouring group is OR-ed into its cleared word (OR does not depend on order)
//   count / offsets / scatter   0xFF bytes per 4 KiB chunk, their scan, the bytes with the inserted zeros, each frame's final length
#include <cstdint>

#include "common.h"

namespace jenc {

constexpr int GROUP = 32;          // blocks per workgroup of the entropy kernels
constexpr int BLOCK_MAX_BITS = 1658;   // DC 9 + 11, 63 x (AC 16 + 10)
constexpr int BLOCK_MAX_BYTES = 208;
constexpr int CHUNK = 4096;        // unstuffed bytes per workgroup of the stuffing kernels
constexpr int LDS_WORDS = (GROUP * BLOCK_MAX_BITS + 31 + 8 + 31) / 32 + 3;

struct QTabs {
    unsigned short d[2][64];   // 8 q, natural order
};

struct HuffSpec {
    unsigned char bits[16];
    unsigned char vals[162];
    int n;
};

constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};

// entry of a code table: (code << 5) | length; 0 = no such symbol
struct HuffTables {
    unsigned ac[2][256];
    unsigned dc[2][16];
};

constexpr void fill_codes(unsigned* table, const HuffSpec& s) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < s.bits[len - 1]; i++) table[s.vals[k++]] = (code++ << 5) | (unsigned)len;
        code <<= 1;
    }
}

constexpr HuffTables make_tables() {
    HuffTables t{};
    fill_codes(t.ac[0], AC_LUMA);
    fill_codes(t.ac[1], AC_CHROMA);
    fill_codes(t.dc[0], DC_LUMA);
    fill_codes(t.dc[1], DC_CHROMA);
    return t;
}

__constant__ HuffTables c_huff = make_tables();

// position in the zigzag scan of the coefficient at natural index i
__constant__ unsigned char c_zigzag_pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                               10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ---- blocks ---------------------------------------------------------------------------------------------------------------------------
// one pass of libjpeg's jfdctint ("islow"), CONST_BITS 13, PASS1_BITS 2
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(const int (&d)[8], int (&o)[8]) {
    constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137, F1_961 = 16069,
                  F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * F0_541;
    o[2] = (z1 + t13 * F0_765 + R) >> N;
    o[6] = (z1 - t12 * F1_847 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1_175;
    t4 *= F0_298;
    t5 *= F2_053;
    t6 *= F3_072;
    t7 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 = z3 * -F1_961 + z5;
    z4 = z4 * -F0_390 + z5;
    o[7] = (t4 + z1 + z3 + R) >> N;
    o[5] = (t5 + z2 + z4 + R) >> N;
    o[3] = (t6 + z2 + z3 + R) >> N;
    o[1] = (t7 + z1 + z4 + R) >> N;
}

// sample (row r, column c) of block b in the DCT work area: lanes that walk (b, r) with c fixed, or (b, c) with r fixed, hit 64 different banks
__device__ __forceinline__ int work_at(int b, int r, int c) { return b * 72 + r + 9 * c; }

__global__ __launch_bounds__(256) void enc_blocks_kernel(const unsigned char* __restrict__ rgb, int H, int W, int MW, int MH, QTabs qt, short* __restrict__ coef,
                                                         int dwords) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[16 * 192];
    __shared__ int work[24 * 72];
    __shared__ __attribute__((aligned(4))) short q[24 * 64];
    __shared__ unsigned short dq[128];
    const int tid = threadIdx.x, bx = blockIdx.x, by = blockIdx.y, f = blockIdx.z;
    const int x0 = bx * 64, y0 = by * 16;
    const int Hs = min(16, H - y0), Ws = min(64, W - x0);   // the source pixels under this strip: both >= 1
    const size_t pitch = (size_t)3 * W;
    const unsigned char* src = rgb + ((size_t)f * H + y0) * pitch + (size_t)x0 * 3;
    const int row_bytes = 3 * Ws;
    if (tid < 128) dq[tid] = qt.d[tid >> 6][tid & 63];
    if (dwords) {   // 3 W is a multiple of 4 and so is the base address: every row and every strip starts on a dword, and a row ends on one
        const int nd = row_bytes >> 2;
        for (int i = tid; i < Hs * 48; i += 256) {
            const int r = i / 48, c = i % 48;
            if (c < nd) reinterpret_cast<unsigned*>(raw)[r * 48 + c] = *reinterpret_cast<const unsigned*>(src + r * pitch + 4 * c);
        }
    } else {
        for (int i = tid; i < Hs * 192; i += 256) {
            const int r = i / 192, c = i % 192;
            if (c < row_bytes) raw[r * 192 + c] = src[r * pitch + c];
        }
    }
    __syncthreads();
    // one 2 x 2 quad per thread: four luma samples (edge-replicated by clamping) and one sample of each chroma plane
    const int qy = tid >> 5, qx = tid & 31;
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int py = 2 * qy + dy, px = 2 * qx + dx;
            const unsigned char* p = &raw[min(py, Hs - 1) * 192 + min(px, Ws - 1) * 3];
            const int y = (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
            work[work_at((px >> 4) * 6 + ((py >> 3) << 1) + ((px >> 3) & 1), py & 7, px & 7)] = y - 128;
        }
    }
    {
        // chroma rows past the last downsampled row repeat THAT row (libjpeg pads the downsampled plane, not the source); columns past the
        // source repeat its last column; an odd height repeats the last source row once
        const int cq = min(qy, ((H + 1) >> 1) - 8 * by - 1);
        const int r0 = 2 * cq, r1 = min(2 * cq + 1, Hs - 1), c0 = min(2 * qx, Ws - 1), c1 = min(2 * qx + 1, Ws - 1);
        int cb = 0, cr = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned char* p = &raw[((k & 2) ? r1 : r0) * 192 + ((k & 1) ? c1 : c0) * 3];
            const int R = p[0], G = p[1], B = p[2];
            cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        }
        const int bias = 1 + (qx & 1);
        work[work_at((qx >> 3) * 6 + 4, qy, qx & 7)] = ((cb + bias) >> 2) - 128;
        work[work_at((qx >> 3) * 6 + 5, qy, qx & 7)] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    int d[8], o[8];
    if (tid < 192) {   // rows, in place
        const int b = tid >> 3, r = tid & 7;
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = work[work_at(b, r, k)];
        fdct_pass<true>(d, o);
#pragma unroll
        for (int k = 0; k < 8; k++) work[work_at(b, r, k)] = o[k];
    }
    __syncthreads();
    if (tid < 192) {   // columns, quantisation
        const int b = tid >> 3, c = tid & 7;
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = work[work_at(b, k, c)];
        fdct_pass<false>(d, o);
        const unsigned short* div = &dq[(b % 6) < 4 ? 0 : 64];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int nat = 8 * k + c;
            const unsigned dv = div[nat], a = (unsigned)abs(o[k]);
            const int m = (int)((a + (dv >> 1)) / dv);
            q[b * 64 + c_zigzag_pos[nat]] = (short)(o[k] < 0 ? -m : m);
        }
    }
    __syncthreads();
    // out: the strip's MCUs lie back to back.  A dummy luma block (past the image's block columns or rows) has no AC and the DC of the block
    // before it in the MCU, which resolves to a real block of the same MCU
    const int nm = min(4, MW - 4 * bx), BW = (W + 7) >> 3, BH = (H + 7) >> 3;
    unsigned* dst = reinterpret_cast<unsigned*>(coef + (((size_t)f * MH + by) * MW + 4 * bx) * 384);
    for (int i = tid; i < nm * 192; i += 256) {
        const int s0 = 2 * i, b = s0 >> 6, k = s0 & 63, m = b / 6, j = b % 6;
        short v0 = q[s0], v1 = q[s0 + 1];
        if (j < 4) {
            const int gx0 = 2 * (4 * bx + m);
            const bool drow = 2 * by + (j >> 1) >= BH, dcol = gx0 + (j & 1) >= BW;
            if (drow || dcol) {
                const int sj = drow ? (gx0 + 1 < BW ? 1 : 0) : j - 1;
                v0 = k == 0 ? q[(m * 6 + sj) * 64] : (short)0;
                v1 = 0;
            }
        }
        dst[i] = (unsigned)(unsigned short)v0 | ((unsigned)(unsigned short)v1 << 16);
    }
}

// ---- entropy coding -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int magnitude_bits(int v) { return 32 - __clz(abs(v)); }   // 0 for 0

__device__ __forceinline__ void append(unsigned long long& code, int& len, unsigned entry) {
    code = (code << (entry & 31)) | (entry >> 5);
    len += entry & 31;
}

// the bits lane `lane` of a block's wave contributes: lane 0 the DC difference, a lane with a non-zero coefficient its ZRLs, run/size code and
// value bits, lane 63 the EOB if the block ends in a zero.  At most 3 x 11 + 16 + 10 = 59 bits.
__device__ __forceinline__ void lane_symbol(int lane, int v, int diff, const unsigned* ac, const unsigned* dc, unsigned long long& code, int& len) {
    const unsigned long long mask = __ballot(lane > 0 && v != 0);
    code = 0;
    len = 0;
    if (lane == 0) {
        const int s = magnitude_bits(diff);
        append(code, len, dc[s]);
        code = (code << s) | (unsigned)((diff < 0 ? diff - 1 : diff) & ((1 << s) - 1));
        len += s;
    } else if (v != 0) {
        const unsigned long long below = mask & ((1ull << lane) - 1);
        const int prev = below ? 63 - __clzll((long long)below) : 0;
        const int run = lane - prev - 1, s = magnitude_bits(v);
        for (int i = 0; i < (run >> 4); i++) append(code, len, ac[0xF0]);
        append(code, len, ac[((run & 15) << 4) | s]);
        code = (code << s) | (unsigned)((v < 0 ? v - 1 : v) & ((1 << s) - 1));
        len += s;
    } else if (lane == 63) {
        append(code, len, ac[0]);
    }
}

// block `blk` of a frame (scan order: six per MCU) -> the quantised DC its difference is taken from (0 at the start of the frame)
__device__ __forceinline__ int predictor(const short* __restrict__ coef, long long blk) {
    const int j = (int)(blk % 6);
    long long p;
    if (j >= 4) p = blk - 6;
    else if (j > 0) p = blk - 1;
    else p = blk - 3;   // Y00: Y11 of the MCU before
    return p < 0 ? 0 : coef[p * 64];
}

__device__ __forceinline__ void load_tables(unsigned* ac, unsigned* dc) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) ac[i] = c_huff.ac[i >> 8][i & 255];
    if (threadIdx.x < 32) dc[threadIdx.x] = c_huff.dc[threadIdx.x >> 4][threadIdx.x & 15];
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_inclusive(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(256) void enc_bits_kernel(const short* __restrict__ coef, long long NB, int NG, int* __restrict__ bits, unsigned* __restrict__ gtot) {
    __shared__ unsigned ac[512], dc[32];
    __shared__ int wsum[4];
    load_tables(ac, dc);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.x, f = blockIdx.y;
    const short* fc = coef + (size_t)f * NB * 64;
    int total = 0;
    for (int i = 0; i < 8; i++) {
        const long long blk = (long long)g * GROUP + wave * 8 + i;
        if (blk >= NB) break;   // (uniform over the wave)
        const int v = fc[blk * 64 + lane];
        const int diff = lane == 0 ? v - predictor(fc, blk) : 0;
        const int tab = (blk % 6) < 4 ? 0 : 1;
        unsigned long long code;
        int len;
        lane_symbol(lane, v, diff, ac + 256 * tab, dc + 16 * tab, code, len);
        const int b = wave_sum(len);
        if (lane == 0) bits[(size_t)f * NB + blk] = b;
        total += b;
    }
    if (lane == 0) wsum[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) gtot[(size_t)f * NG + g] = (unsigned)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// exclusive scan of 256 values of one workgroup (one per thread); returns the exclusive prefix and the total through `sum`
template <typename T>
__device__ __forceinline__ T block_exclusive(T v, T* wtot, T& sum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();   // (wtot may still be read from the call before)
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    T before = 0;
    for (int w = 0; w < wave; w++) before += wtot[w];
    sum = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    return before + inc - v;
}

__global__ __launch_bounds__(256) void enc_offsets_kernel(const unsigned* __restrict__ gtot, int NG, unsigned long long* __restrict__ goff, unsigned* __restrict__ ubytes,
                                                          unsigned* __restrict__ stream, size_t stream_words) {
    __shared__ unsigned long long wtot[4];
    const int f = blockIdx.x;
    unsigned* us = stream + (size_t)f * stream_words;
    unsigned long long carry = 0;
    for (int g0 = 0; g0 < NG; g0 += 256) {
        const int g = g0 + threadIdx.x;
        const unsigned long long v = g < NG ? gtot[(size_t)f * NG + g] : 0;
        unsigned long long sum;
        const unsigned long long off = carry + block_exclusive<unsigned long long>(v, wtot, sum);
        if (g < NG) {
            goff[(size_t)f * NG + g] = off;
            us[off >> 5] = 0;   // the word this group shares with the one before it
        }
        carry += sum;
    }
    if (threadIdx.x == 0) {
        if (carry & 31) us[carry >> 5] = 0;   // the last, partly filled word (if the frame ends on a word, the scan above cleared nothing past it)
        ubytes[f] = (unsigned)((carry + 7) >> 3);
    }
}

__device__ __forceinline__ void put_bits(unsigned* buf, unsigned pos, int len, unsigned long long code) {
    if (len == 0) return;
    const unsigned long long v = code << (64 - len);   // left-aligned
    const unsigned w = pos >> 5, sh = pos & 31;
    const unsigned long long hi = v >> sh;
    const unsigned w0 = (unsigned)(hi >> 32), w1 = (unsigned)hi, w2 = sh ? (unsigned)((v << (64 - sh)) >> 32) : 0u;
    if (w0) atomicOr(&buf[w], w0);
    if (w1) atomicOr(&buf[w + 1], w1);
    if (w2) atomicOr(&buf[w + 2], w2);
}

__global__ __launch_bounds__(256) void enc_emit_kernel(const short* __restrict__ coef, long long NB, int NG, const int* __restrict__ bits, const unsigned* __restrict__ gtot,
                                                       const unsigned long long* __restrict__ goff, unsigned* __restrict__ stream, size_t stream_words) {
    __shared__ unsigned ac[512], dc[32];
    __shared__ unsigned buf[LDS_WORDS];
    __shared__ int boff[GROUP];
    load_tables(ac, dc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x, f = blockIdx.y;
    for (int i = tid; i < LDS_WORDS; i += 256) buf[i] = 0;
    if (wave == 0) {
        const long long blk = (long long)g * GROUP + lane;
        const int b = (lane < GROUP && blk < NB) ? bits[(size_t)f * NB + blk] : 0;
        const int inc = wave_inclusive(b, lane);
        if (lane < GROUP) boff[lane] = inc - b;
    }
    __syncthreads();
    const short* fc = coef + (size_t)f * NB * 64;
    const unsigned long long start = goff[(size_t)f * NG + g];
    const unsigned gbits = gtot[(size_t)f * NG + g], align = (unsigned)(start & 31);
    for (int i = 0; i < 8; i++) {
        const int lb = wave * 8 + i;
        const long long blk = (long long)g * GROUP + lb;
        if (blk >= NB) break;
        const int v = fc[blk * 64 + lane];
        const int diff = lane == 0 ? v - predictor(fc, blk) : 0;
        const int tab = (blk % 6) < 4 ? 0 : 1;
        unsigned long long code;
        int len;
        lane_symbol(lane, v, diff, ac + 256 * tab, dc + 16 * tab, code, len);
        const int at = wave_inclusive(len, lane) - len;
        put_bits(buf, align + boff[lb] + at, len, code);
    }
    unsigned end = align + gbits;
    if (g == NG - 1) {   // the frame's last byte is filled with 1-bits
        const int pad = (int)((8 - ((start + gbits) & 7)) & 7);
        if (tid == 0) put_bits(buf, end, pad, (1ull << pad) - 1);
        end += pad;
    }
    __syncthreads();
    unsigned* us = stream + (size_t)f * stream_words + (start >> 5);
    const unsigned nwords = (end + 31) >> 5;
    for (unsigned w = tid; w < nwords; w += 256) {
        const unsigned val = __builtin_bswap32(buf[w]);   // bits go MSB first, the stream is bytes
        // the first word may hold the end of the group before, the last one the start of the group after: both were cleared by the offsets
        // kernel and take an OR; every other word is this group's alone
        if (w == 0 || (w == nwords - 1 && (end & 31)))
            atomicOr(&us[w], val);
        else
            us[w] = val;
    }
}

// ---- byte stuffing --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int load16(const unsigned char* us, unsigned at, unsigned L, unsigned char (&b)[16]) {
    const uint4 v = *reinterpret_cast<const uint4*>(us + at);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    int n = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        b[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
        n += (at + k < L && b[k] == 0xFF) ? 1 : 0;
    }
    return n;
}

__global__ __launch_bounds__(256) void enc_count_kernel(const unsigned* __restrict__ stream, size_t stream_words, const unsigned* __restrict__ ubytes, int NC,
                                                        unsigned* __restrict__ cnt) {
    __shared__ int wsum[4];
    const int f = blockIdx.y, c = blockIdx.x;
    const unsigned L = ubytes[f];
    if ((unsigned long long)c * CHUNK >= L) return;
    unsigned char b[16];
    const int n = wave_sum(load16(reinterpret_cast<const unsigned char*>(stream + (size_t)f * stream_words), c * CHUNK + threadIdx.x * 16, L, b));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(size_t)f * NC + c] = (unsigned)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void enc_stuff_offsets_kernel(unsigned* __restrict__ cnt, int NC, const unsigned* __restrict__ ubytes, size_t capacity,
                                                                long long* __restrict__ sizes, int* __restrict__ status) {
    __shared__ unsigned wtot[4];
    const int f = blockIdx.x;
    const unsigned L = ubytes[f];
    const int nc = (int)(((unsigned long long)L + CHUNK - 1) / CHUNK);
    unsigned carry = 0;
    for (int c0 = 0; c0 < nc; c0 += 256) {
        const int c = c0 + threadIdx.x;
        const unsigned v = c < nc ? cnt[(size_t)f * NC + c] : 0;
        unsigned sum;
        const unsigned off = carry + block_exclusive<unsigned>(v, wtot, sum);
        if (c < nc) cnt[(size_t)f * NC + c] = off;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        const unsigned long long size = (unsigned long long)L + carry;
        sizes[f] = (long long)size;
        status[f] = size > capacity ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void enc_scatter_kernel(const unsigned* __restrict__ stream, size_t stream_words, const unsigned* __restrict__ ubytes, int NC,
                                                          const unsigned* __restrict__ coff, unsigned char* __restrict__ out, size_t capacity) {
    __shared__ int wtot[4];
    const int f = blockIdx.y, c = blockIdx.x;
    const unsigned L = ubytes[f];
    if ((unsigned long long)c * CHUNK >= L) return;   // (uniform over the workgroup)
    unsigned char b[16];
    const unsigned at = c * CHUNK + threadIdx.x * 16;
    const int n = load16(reinterpret_cast<const unsigned char*>(stream + (size_t)f * stream_words), at, L, b);
    int sum;
    const int before = block_exclusive<int>(n, wtot, sum);
    unsigned char* slot = out + (size_t)f * capacity;
    size_t pos = (size_t)at + coff[(size_t)f * NC + c] + before;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (at + k >= L) break;
        if (pos < capacity) slot[pos] = b[k];
        pos++;
        if (b[k] == 0xFF) {
            if (pos < capacity) slot[pos] = 0;
            pos++;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    long long NB;          // blocks per frame
    int MW, MH, NG, NC;    // MCU columns and rows, groups, stuffing chunks per frame
    size_t stream_bytes;   // per frame: the unstuffed stream's worst case, a multiple of 256
    size_t coef, bits, gtot, goff, ubytes, stream, cnt, total;

    Layout(int n, int w, int h) {
        MW = (w + 15) / 16;
        MH = (h + 15) / 16;
        NB = 6LL * MW * MH;
        NG = (int)((NB + GROUP - 1) / GROUP);
        stream_bytes = up256((size_t)NB * BLOCK_MAX_BYTES + 64);
        NC = (int)((stream_bytes + CHUNK - 1) / CHUNK);
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t here = at;
            at += up256(bytes);
            return here;
        };
        coef = take((size_t)n * NB * 64 * sizeof(short));
        bits = take((size_t)n * NB * sizeof(int));
        gtot = take((size_t)n * NG * sizeof(unsigned));
        goff = take((size_t)n * NG * sizeof(unsigned long long));
        ubytes = take((size_t)n * sizeof(unsigned));
        stream = take((size_t)n * stream_bytes + CHUNK);   // (the stuffing kernels read whole 16-byte pieces up to the chunk's end)
        cnt = take((size_t)n * NC * sizeof(unsigned));
        total = at;
    }
};

// a frame whose worst-case scan (every byte stuffed) cannot be addressed with 32 bits is refused
inline bool fits32(int w, int h) {
    const long long nb = 6LL * ((w + 15) / 16) * ((h + 15) / 16);
    return 2 * (nb * BLOCK_MAX_BYTES + 64) + CHUNK < (1LL << 32);
}

}  // namespace jenc

extern "C" {

size_t df3d_jpeg_encode_work_bytes(int n, int w, int h) {
    if (n < 0 || w < 1 || h < 1 || w > 65535 || h > 65535 || !jenc::fits32(w, h)) return 0;
    return jenc::Layout(n, w, h).total;
}

int df3d_jpeg_encode_rgb(const unsigned char* rgb_dev, int n, int h, int w, const unsigned char* qtab_luma, const unsigned char* qtab_chroma, unsigned char* out_dev,
                         size_t out_capacity_per_frame, long long* sizes_dev, int* status_dev, void* work_dev, size_t work_bytes, short* coef_out_dev,
                         int* bits_out_dev, void* stream) {
    using namespace jenc;
    DF3D_CHECK_ARG(n >= 0, "n must not be negative");
    DF3D_CHECK_ARG(w >= 1 && w <= 65535 && h >= 1 && h <= 65535, "width and height must be 1 .. 65535");
    if (n == 0) return DF3D_OK;
    DF3D_CHECK_ARG(rgb_dev && qtab_luma && qtab_chroma && out_dev && sizes_dev && status_dev && work_dev, "null pointer");
    QTabs qt;
    for (int i = 0; i < 64; i++) {
        DF3D_CHECK_ARG(qtab_luma[i] >= 1 && qtab_chroma[i] >= 1, "quantisation table entries must be 1 .. 255");
        qt.d[0][i] = (unsigned short)(8 * qtab_luma[i]);
        qt.d[1][i] = (unsigned short)(8 * qtab_chroma[i]);
    }
    DF3D_CHECK_ARG(fits32(w, h), "frame too large: its worst-case scan does not fit 32-bit offsets");
    DF3D_CHECK_ARG(((uintptr_t)work_dev & 255) == 0, "work_dev must be 256-byte aligned");
    DF3D_CHECK_ARG(work_bytes >= df3d_jpeg_encode_work_bytes(n, w, h), "work buffer too small (df3d_jpeg_encode_work_bytes)");
    DF3D_CHECK_ARG(!coef_out_dev || ((uintptr_t)coef_out_dev & 3) == 0, "coef_out_dev must be 4-byte aligned");
    const Layout L(n, w, h);
    hipStream_t s = df3d::as_stream(stream);
    char* wk = static_cast<char*>(work_dev);
    short* coef = coef_out_dev ? coef_out_dev : reinterpret_cast<short*>(wk + L.coef);
    int* bits = bits_out_dev ? bits_out_dev : reinterpret_cast<int*>(wk + L.bits);
    unsigned* gtot = reinterpret_cast<unsigned*>(wk + L.gtot);
    unsigned long long* goff = reinterpret_cast<unsigned long long*>(wk + L.goff);
    unsigned* ubytes = reinterpret_cast<unsigned*>(wk + L.ubytes);
    unsigned* ustream = reinterpret_cast<unsigned*>(wk + L.stream);
    unsigned* cnt = reinterpret_cast<unsigned*>(wk + L.cnt);
    const size_t stream_words = L.stream_bytes / 4;
    const int dwords = ((3LL * w) % 4 == 0 && ((uintptr_t)rgb_dev & 3) == 0) ? 1 : 0;
    const size_t frame_bytes = (size_t)3 * w * h;
    for (int f0 = 0; f0 < n; f0 += 32768) {   // (a grid's y and z extents end at 65535)
        const int m = n - f0 < 32768 ? n - f0 : 32768;
        short* cf = coef + (size_t)f0 * L.NB * 64;
        int* bt = bits + (size_t)f0 * L.NB;
        unsigned *gt = gtot + (size_t)f0 * L.NG, *ub = ubytes + f0, *us = ustream + (size_t)f0 * stream_words, *cn = cnt + (size_t)f0 * L.NC;
        unsigned long long* go = goff + (size_t)f0 * L.NG;
        hipLaunchKernelGGL(enc_blocks_kernel, dim3((L.MW + 3) / 4, L.MH, m), dim3(256), 0, s, rgb_dev + f0 * frame_bytes, h, w, L.MW, L.MH, qt, cf, dwords);
        hipLaunchKernelGGL(enc_bits_kernel, dim3(L.NG, m), dim3(256), 0, s, cf, L.NB, L.NG, bt, gt);
        hipLaunchKernelGGL(enc_offsets_kernel, dim3(m), dim3(256), 0, s, gt, L.NG, go, ub, us, stream_words);
        hipLaunchKernelGGL(enc_emit_kernel, dim3(L.NG, m), dim3(256), 0, s, cf, L.NB, L.NG, bt, gt, go, us, stream_words);
        hipLaunchKernelGGL(enc_count_kernel, dim3(L.NC, m), dim3(256), 0, s, us, stream_words, ub, L.NC, cn);
        hipLaunchKernelGGL(enc_stuff_offsets_kernel, dim3(m), dim3(256), 0, s, cn, L.NC, ub, out_capacity_per_frame, sizes_dev + f0, status_dev + f0);
        hipLaunchKernelGGL(enc_scatter_kernel, dim3(L.NC, m), dim3(256), 0, s, us, stream_words, ub, L.NC, cn, out_dev + (size_t)f0 * out_capacity_per_frame,
                           out_capacity_per_frame);
    }
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

}  // extern "C"
