"""-m gpu: every hourglass plan step against a TEACHER-FORCED float64 oracle (oracle/hourglass_torch.py forward_traced with
`forced` = the device's own earlier steps, oracle/hg_local.py for the figures).

tests/test_gpu_hourglass.py runs the oracle from the image and compares step k relative to the tensor's max magnitude, so
every step carries the error of all the steps before it.  Here the oracle computes step k from the DEVICE's outputs of
the earlier steps, in float64 with the engine's own (folded, float32) parameters, and every element is judged against
its own magnitude scale -- the same layer on the magnitudes of the operands it reads.  Figures (oracle/hg_local.py) and
bounds, with the worst step measured on the MI355X over the whole matrix below (5 engines x 2 plans x 5 shapes, and the
fuse_upadd 0 / 2 and register-staged plans at 256 x 512):
    float32 storage, max |got - ref| / (2^-24 * scale), one constant per kernel family:
        direct (f32 wino=0, every unfused f32 plan)    32   (measured 11.5)
        Winograd (f32 default)                         32   (measured 9.9)
        f32s (IEEE-half split products)                48   (measured 15.5, hg.0.hg.3.2.0.conv3)
    bf16 / f16 against round_T(float64 layer on T-rounded operands, rounded where the kernels round), per step:
        max ulp                 unfused 1.5 (measured 1.0: one rounding flip); fused 4 (measured 2.0, an f16 ADD2 sum:
                                the unit there is floored at u_T * scale for the inner t1 / t2 roundings)
        bit-identical fraction  unfused >= 0.98 (measured 0.996 on the large steps, 0.985 on a 512-element innermost step);
                                fused >= 0.97 (measured 0.992); both less 4 binomial standard errors
        |mean signed error|     <= 0.02 + 4 standard errors (measured 0.0147 on that 512-element step, < 0.005 on the large
                                steps; a truncating conversion: -0.6)
    pools, and up-adds of two stored tensors: bit-identical to the model (measured: 0 elements differ).  The up-add the ADD2
    epilogue writes (fuse_upadd=1) is a fused step and held to the fused bounds.
The simulated bugs of tests/test_oracle_forced.py (truncation, a dropped bias, a padding row, a tile column, a missing ReLU,
one channel 4 ulps off, a fused bottleneck's tile column 16 ulps off) fail these bounds.  The whole matrix runs in about two
minutes.
"""
import re

import pytest
import torch

from oracle import hg_local as hl
from oracle import hourglass_torch as oh

pytestmark = pytest.mark.gpu

FINAL = f"score.{oh.NUM_STACKS - 1}"
DTYPES = {   # name: (engine dtype, engine options)
    "f32": ("f32", {}),
    "f32-direct": ("f32", {"wino": 0}),
    "f32s": ("f32s", {}),
    "bf16": ("bf16", {}),
    "f16": ("f16", {}),
}
SHAPES = [(256, 512, 2), (192, 320, 1), (128, 64, 2), (64, 64, 1), (64, 512, 1)]
PLANS = {"default": {}, "unfused": {"fuse": False}}
EXTRA = {"upadd0": {"fuse_upadd": 0}, "upadd2": {"fuse_upadd": 2}, "register-staged": {"ring": False, "l1": False}}
CONFIGS = [(d, p, s) for d in DTYPES for p in PLANS for s in SHAPES] + [(d, p, SHAPES[0]) for d in DTYPES for p in EXTRA]


@pytest.fixture(scope="module")
def oracle_net():
    torch.manual_seed(0)
    return oh.build(seed=0)


def _oracle_name(name, got, height):
    """The oracle's name for what a plan step stores, where the plan names it otherwise:
    * the layer1 kernel that writes only the pooled tensor: step "layer1.0.conv3" holds "maxpool";
    * a level whose bottleneck cannot take the pending up-path sum in its input load (a level below the fused kernels'
      8 x 16 tile) materialises it first under the CONSUMER's name: "hg.S.hg.L.2.0.upadd" is level L-1's sum
      "hg.S.hg.{L-1}.upadd", "res.S.0.upadd" the outermost level's."""
    if name == "layer1.0.conv3" and got.shape[1] == height // 4:
        return "maxpool"
    m = re.fullmatch(r"(hg\.\d+\.hg\.)(\d+)\.2\.0\.upadd", name)
    if m:
        return f"{m.group(1)}{int(m.group(2)) - 1}.upadd"
    m = re.fullmatch(r"res\.(\d+)\.0\.upadd", name)
    if m:
        return f"hg.{m.group(1)}.hg.{oh.DEPTH - 1}.upadd"
    return name


def _family(dtype_key, opts, name, A):
    if A.storage != "f32":
        return "fused" if name in A.fused or name.endswith(("pool", "upadd")) else "unfused"
    if dtype_key == "f32s":
        return "f32s"
    return "wino" if dtype_key == "f32" and opts.get("fuse", True) else "direct"


@pytest.mark.parametrize("dtype_key,plan,shape", CONFIGS, ids=[f"{d}-{p}-{h}x{w}x{n}" for d, p, (h, w, n) in CONFIGS])
def test_every_step_against_forced_oracle(native_lib, cuda, oracle_net, dtype_key, plan, shape):
    from deepfly3d_amd.hourglass import HourglassEngine

    height, width, n = shape
    dtype, opts = DTYPES[dtype_key]
    opts = dict(opts, **PLANS.get(plan, EXTRA.get(plan)))
    eng = HourglassEngine(oracle_net.state_dict(), dtype=dtype, device=cuda, height=height, width=width, **opts)
    img = torch.rand((n, height, width, 3), generator=torch.Generator().manual_seed(11 * height + width + n), dtype=torch.float32)
    x = img.to(cuda)
    dev = {}
    for k, (name, hwc) in enumerate(eng.steps(), start=1):
        eng._workspace(n).fill_(0xFF)   # NaN-poisoned workspace: a step reading memory this forward has not written shows it
        got = eng.forward_upto(x, k).cpu()
        name = _oracle_name(name, got, height)
        assert name not in dev, name
        dev[name] = got
    assert FINAL in dev and list(dev)[-1] == FINAL
    A = oh.Arith(oracle_net, "f32" if dtype in ("f32", "f32s") else dtype)
    ref = oh.forward_traced(oracle_net, img, forced={k: v for k, v in dev.items() if k != FINAL}, arith=A)
    assert set(dev) <= set(ref), set(dev) - set(ref)

    bad, worst = [], {}
    for name, got in dev.items():
        assert tuple(got.shape) == tuple(ref[name].shape), (name, got.shape, ref[name].shape)
        exact = name in A.exact
        fam = "exact" if exact else _family(dtype_key, opts, name, A)
        fig = hl.figures(got, ref[name], A.scale[name], A.storage, exact=exact, rounded=name != FINAL, fused=fam == "fused")
        for v in hl.violations(fig, A.storage, fam):
            bad.append(f"{name} [{fam}]: {v}")
        for key, val in fig.items():
            if key in ("max_abs", "bias_se", "n"):
                continue
            w = worst.get((fam, key))
            if w is None or (abs(val) < abs(w[0]) if key == "equal" else abs(val) > abs(w[0])):
                worst[(fam, key)] = (val, name)
    summary = ", ".join(f"{fam} {key} {val:.3g} ({name})" for (fam, key), (val, name) in sorted(worst.items()))
    print(f"\n{dtype_key} {plan} {height}x{width}x{n}: {len(dev)} steps; worst: {summary}")
    assert not bad, "\n".join(bad[:20])
