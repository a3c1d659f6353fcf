"""Local error figures of one hourglass plan step against the teacher-forced oracle (hourglass_torch.forward_traced with
`forced` = the device's own earlier outputs and an `Arith`).  TEST INFRASTRUCTURE ONLY -- the product never imports it.

Every figure is dimensionless and element-wise, so a kernel that is wrong on one border column, one channel or by a
biased rounding shows up at full size instead of under the max-magnitude of a whole tensor:
  * float32 storage (f32, f32s): err = max |got - ref| / (u32 * scale), u32 = 2^-24, scale = the same layer on absolute
    values (conv(|a|, |w|) + |b| (+ |skip|)): the forward error bound of a float32 dot product is a small multiple of it.
  * bf16 / f16 storage, against round_T(the layer in float64 on T-rounded operands):
      ulp   = max |got - ref| / max(ulp_T(ref), floor): ulps of T.  Single-convolution steps: floor = LP_FLOOR * u32 * scale,
              the float32 accumulation allowance (FP32_ERR["direct"]), which matters only where the result cancels ~2^16
              below its operands.  Fused steps (an inner T rounding of the device, t1 / t2 / y, was not forced and can
              differ from the model's by one ulp): floor = u_T * scale, what such a difference carries into the output
      equal = the fraction of the elements (either side non-zero) that are bit-identical; its floor is lowered by 4 binomial
              standard errors on a step of n elements, as the bias bound below is widened
      bias  = the mean signed error in ulps, (|got| - |ref|) / ulp_T(ref) clipped to [-1, 1]: ~0 for round-to-nearest-even,
              about -0.5 for a conversion that truncates; bias_se = its standard error (a step of a few hundred elements
              -- the innermost levels of a small image -- has a noisy mean)
  * steps without a product (pools, up-adds, whose inputs were all forced): bit-identical.
The bounds are stated here, next to what the MI355X measured, so that the CPU self-test (tests/test_oracle_forced.py) holds
its simulated mutants to the same numbers as the GPU test (tests/test_gpu_hourglass_local.py)."""
import torch

from .hourglass_torch import STORAGE_BITS

# float32-storage engines: max err per kernel family (a few times the measured worst step; see tests/test_gpu_hourglass_local.py)
FP32_ERR = {"direct": 32.0, "wino": 32.0, "f32s": 48.0}
# 16-bit engines: max ulp (unfused: one rounding of a float32 accumulator can land one ulp away and no further; fused: a few times
# the measured 2.0), min fraction bit-identical (less 4 standard errors), max |mean signed ulp| (plus 4 standard errors of the mean)
LP_ULP = {"unfused": 1.5, "fused": 4.0}
LP_EQUAL = {"unfused": 0.98, "fused": 0.97}
LP_BIAS = 0.02
LP_BIAS_SE = 4.0
LP_FLOOR = FP32_ERR["direct"]


def ulp(v, storage):
    """Unit in the last place of |v| in the storage format (0 where v == 0; IEEE half's subnormal spacing below 2^-14)."""
    p = STORAGE_BITS[storage]
    _, e = torch.frexp(v.abs().double())   # |v| = m 2^e, m in [0.5, 1): ulp = 2^(e - p)
    if storage == "f16":
        e = e.clamp_min(-13)
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - p))


def _ratio(num, den):
    return torch.where(num == 0, torch.zeros_like(num), num / den)


def figures(got, ref, scale, storage, exact=False, rounded=True, fused=False):
    """Figures of one step: got (device), ref (forced oracle, float64), scale (float64), all the same shape.
    exact: a step without a product (bit-identity).  rounded: the 16-bit step's output is stored in T (False for the
    final float32 heat-maps).  fused: the step has inner roundings the oracle did not force (the 16-bit ulp floor)."""
    got, ref, scale = got.double(), ref.double(), scale.double()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    d = (got - ref).abs()
    if exact:
        return {"mismatch": int((d != 0).sum()) + int(torch.isnan(got).sum()), "max_abs": float(d.max())}
    if not bool(torch.isfinite(got).all()):
        return {"nonfinite": int((~torch.isfinite(got)).sum()), "err": float("inf"), "ulp": float("inf")}
    if storage == "f32":
        return {"err": float(_ratio(d, 2.0**-24 * scale).max())}
    floor = (2.0 ** -STORAGE_BITS[storage] if fused else LP_FLOOR * 2.0**-24) * scale
    unit = torch.maximum(ulp(ref, storage), floor)
    nz = (ref != 0) | (got != 0)
    ul = ulp(torch.where(ref != 0, ref, got), storage)
    signed = _ratio(got.abs() - ref.abs(), ul).clamp(-1.0, 1.0)
    sig = signed[nz]
    out = {"ulp": float(_ratio(d, unit).max()), "bias": float(sig.mean()) if sig.numel() else 0.0,
           "bias_se": float((sig.square().mean() / sig.numel()).sqrt()) if sig.numel() else 0.0}
    if rounded:
        out["equal"] = float((d[nz] == 0).double().mean()) if bool(nz.any()) else 1.0
        out["n"] = int(nz.sum())
    return out


def violations(fig, storage, family):
    """The bounds a step's figures break (an empty list: the step passes).  family: "direct" / "wino" / "f32s" for float32
    storage, "unfused" / "fused" for the 16-bit engines (fused: the step is a fused kernel with roundings inside it)."""
    bad = []
    if "mismatch" in fig:
        if fig["mismatch"]:
            bad.append(f"{fig['mismatch']} elements not bit-identical (max |diff| {fig['max_abs']:.3e})")
        return bad
    if "nonfinite" in fig:
        return [f"{fig['nonfinite']} non-finite elements"]
    if storage == "f32":
        if not fig["err"] <= FP32_ERR[family]:
            bad.append(f"err {fig['err']:.2f} u32*scale > {FP32_ERR[family]}")
        return bad
    if not fig["ulp"] <= LP_ULP[family]:
        bad.append(f"ulp {fig['ulp']:.2f} > {LP_ULP[family]}")
    bias_bound = LP_BIAS + LP_BIAS_SE * fig["bias_se"]
    if not abs(fig["bias"]) <= bias_bound:
        bad.append(f"mean signed error {fig['bias']:+.3f} ulp, |.| > {bias_bound:.3f}")
    if "equal" in fig:
        p = LP_EQUAL[family]
        floor = p - LP_BIAS_SE * (p * (1.0 - p) / max(fig["n"], 1)) ** 0.5
        if not fig["equal"] >= floor:
            bad.append(f"bit-identical fraction {fig['equal']:.3f} < {floor:.3f}")
    return bad
