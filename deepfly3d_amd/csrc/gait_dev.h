// Device helpers that gait.hip (a15) and treadmill.hip (a17) share: three-vectors whose dot product is x x + y y + z z from the left,
// section 14's missing-joint rule, the clipped window of the tip's velocity, and the scaffold of the blocked scans (the scan of one
// block of 256 lanes under any associative operation; a scan along time is three launches on top of it: block results, one block per
// row over the block results with a carry, apply).  Both files are built with -ffp-contract=off (build.py).
#pragma once
#include <cmath>

#include "common.h"

namespace df3d {
namespace gait_dev {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int JOINTS = 38;
constexpr int LEGS = 6;
constexpr int HALF_MIN = 1, HALF_MAX = 64;
constexpr long long T_MAX = 0x7fffffffLL / LEGS;   // 6 T samples are numbered by an int32

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 load3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ bool finite3(V3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// section 14's rule: all three coordinates exactly zero (the DLT's "fewer than two views"), or any of them not finite
__device__ __forceinline__ bool missing(V3 p) { return (p.x == 0.0 && p.y == 0.0 && p.z == 0.0) || !finite3(p); }

// the joint id of leg L's body-coxa P0; the tip P4 is four joints on
__device__ __forceinline__ int coxa_of(int leg) {
    const int side = leg / 3;
    return 19 * side + 5 * (leg - 3 * side);
}

// the clipped window of the central difference at frame t: a = max(t - w, 0), b = min(t + w, T - 1); empty (b = a) where T = 1
__device__ __forceinline__ void window(long long t, int w, long long T, long long& a, long long& b) {
    a = t - w > 0 ? t - w : 0;
    b = t + w < T - 1 ? t + w : T - 1;
}

struct MaxOp {
    __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; }
};
struct SumOp {
    template <typename V>
    __device__ __forceinline__ V operator()(V a, V b) const { return a + b; }
};

// The inclusive scan of v over the block under `op` (Hillis-Steele: in round o a lane takes op(own, the lane o before)); `exclusive`:
// that of the lanes before this one (`identity` for lane 0); `total`: the block's.  lds: THREADS values.
template <typename V, typename Op>
__device__ __forceinline__ V block_scan(V v, V identity, Op op, V* lds, V& exclusive, V& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    V s = v;
    for (int o = 1; o < THREADS; o <<= 1) {
        const V other = t >= o ? lds[t - o] : identity;
        __syncthreads();
        s = op(s, other);
        lds[t] = s;
        __syncthreads();
    }
    exclusive = t ? lds[t - 1] : identity;
    total = lds[THREADS - 1];
    __syncthreads();   // the next call may write lds
    return s;
}

inline long long round64(long long b) { return (b + 63) / 64 * 64; }
inline long long blocks_of(long long n) { return (n + THREADS - 1) / THREADS; }
inline unsigned grid_of(long long n) { return (unsigned)blocks_of(n); }

template <typename P>
P* at(void* work, long long offset) {
    return reinterpret_cast<P*>(static_cast<char*>(work) + offset);
}

}  // namespace gait_dev
}  // namespace df3d
