// a7, robust losses: scipy's rho table per SCALAR residual, z = (f / C)^2, as tests/ba_robust_oracle.py states it.
//   w  = rho'(z)                     the weight of the residual
//   s2 = rho' + 2 z rho''            in closed form per loss, clamped below at EPS = 2^-52; J's row is scaled by s = sqrt(s2), f by w / s
// The operations are the oracle's one by one.  ba.hip is compiled with floating-point contraction, and an explicit -ffp-contract=fast
// disregards `#pragma clang fp contract(off)`; near 1 - z = 0 (cauchy) and 1 - 3 z^2 = 0 (arctan) a product fused into the sum behind it
// would move s2 by many ulp.  So every product that feeds a sum goes through rounded(): an empty statement the compiler cannot look
// through, no instruction.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/df3d_hip.h"

namespace df3d_robust {

constexpr double EPS = 2.220446049250313e-16;   // 2^-52

__device__ __forceinline__ double rounded(double v) {
    asm volatile("" : "+v"(v));
    return v;
}

struct Row {
    double w, s;
};

__device__ __forceinline__ double z_of(double f, double C) {
    const double q = f / C;
    return rounded(q * q);
}

__device__ __forceinline__ Row row(int loss, double f, double C) {
    const double z = z_of(f, C);
    double w = 1.0, s2 = 1.0;
    switch (loss) {
        case DF3D_BA_LOSS_SOFT_L1: {
            const double t = 1.0 + z, r = sqrt(t);
            w = 1.0 / r;
            s2 = 1.0 / rounded(t * r);
            break;
        }
        case DF3D_BA_LOSS_HUBER:
            if (!(z <= 1.0)) {
                w = 1.0 / sqrt(z);
                s2 = EPS;
            }
            break;
        case DF3D_BA_LOSS_CAUCHY: {
            const double t = 1.0 + z;
            w = 1.0 / t;
            s2 = (1.0 - z) / rounded(t * t);
            break;
        }
        case DF3D_BA_LOSS_ARCTAN: {
            const double z2 = rounded(z * z), t = 1.0 + z2;
            w = 1.0 / t;
            s2 = (1.0 - rounded(3.0 * z2)) / rounded(t * t);
            break;
        }
        default:   // DF3D_BA_LOSS_LINEAR
            break;
    }
    Row o;
    o.w = w;
    o.s = sqrt(s2 <= EPS ? EPS : s2);   // (a NaN residual leaves NaN here: it reaches the cost, where the driver looks for it)
    return o;
}

// rho(z); a residual that is not finite gives NaN (arctan alone would turn an infinite residual into a finite cost)
__device__ __forceinline__ double rho(int loss, double f, double C) {
    if (!isfinite(f)) return NAN;
    const double z = z_of(f, C);
    switch (loss) {
        case DF3D_BA_LOSS_SOFT_L1: return 2.0 * (sqrt(1.0 + z) - 1.0);
        case DF3D_BA_LOSS_HUBER: return z <= 1.0 ? z : rounded(2.0 * sqrt(z)) - 1.0;
        case DF3D_BA_LOSS_CAUCHY: return log1p(z);
        case DF3D_BA_LOSS_ARCTAN: return atan(z);
        default: return z;
    }
}

}  // namespace df3d_robust
