"""CPU self-test of the teacher-forced hourglass oracle and its local checker (oracle/hg_local.py), no GPU.

At 64 x 64, one view: forcing every step with the oracle's own trace changes nothing; a simulated device (the engine's
arithmetic in float32 with another summation order, rounded per the 16-bit model) passes every step at the GPU test's
bounds; and each simulated kernel bug below -- the kind of error the max-magnitude tolerances of tests/test_gpu_hourglass.py
cannot see -- fails at least one step."""
import pytest
import torch
import torch.nn.functional as F

from oracle import hg_local as hl
from oracle import hourglass_torch as oh

FINAL = f"score.{oh.NUM_STACKS - 1}"


class _Every:
    def __contains__(self, name):
        return True


def fused_plan(names):
    """The steps a fully fused plan stores: bottleneck outputs, pools, up-adds and the head outputs -- not a bottleneck's
    conv1 / conv2 / downsample, not the head's fc / score / fc_."""
    inner = (".conv1", ".conv2", ".downsample.0")
    return {k for k in names if not (k.endswith(inner) and k != "conv1") and not k.startswith(("fc.", "fc_.")) and not (k.startswith("score.") and k != FINAL)}


class SimDevice(oh.Arith):
    """The engine's arithmetic as an unfused plan (every step stored), in float32, each convolution summed as two halves
    of its input channels: the same model, another summation order -- what a correct kernel looks like to the checker."""

    def __init__(self, net, storage):
        super().__init__(net, storage, dtype=torch.float32)

    def preact(self, name, x):   # fmaf: x * s + t rounded once to float32 (exact in float64 for a 16-bit x)
        return super().preact(name, x.double()).float() if self.storage != "f32" else super().preact(name, x)

    def conv(self, name, a, stride, pad):
        w, b = self.w[name], self.b[name]
        h = max(1, a.shape[1] // 2)
        return F.conv2d(a[:, h:], w[:, h:], None, stride=stride, padding=pad) + F.conv2d(a[:, :h], w[:, :h], b, stride=stride, padding=pad)


class Truncating(SimDevice):
    """bf16 conversions that truncate (round toward zero) instead of rounding to nearest even."""

    def rnd(self, t):
        bits = t.float().view(torch.int32) & ~0xFFFF
        return bits.view(torch.float32).to(t.dtype)

    def rnd_sum(self, t):
        return self.rnd(t)


class BiasDropped(SimDevice):
    """One output channel of one convolution without its bias (the channel with the largest |bias|)."""

    STEP = "layer3.0.conv3"

    def conv(self, name, a, stride, pad):
        y = super().conv(name, a, stride, pad)
        if name == self.STEP:
            c = int(self.b[name].abs().argmax())
            y[:, c] -= self.b[name][c]
        return y


class BottomPadOffByOne(SimDevice):
    """A 3x3 convolution whose bottom zero-padding row reads the last image row instead."""

    STEP = "layer2.0.conv2"

    def conv(self, name, a, stride, pad):
        if name != self.STEP:
            return super().conv(name, a, stride, pad)
        ap = F.pad(a, (1, 1, 1, 1))
        ap[:, :, -1] = ap[:, :, -2]
        return super().conv(name, ap, stride, 0)


class TileColumnFromNeighbour(SimDevice):
    """The last column of the first 16-wide tile written with its right neighbour's values."""

    STEP = "layer1.0.conv3"

    def post(self, name, t):
        if name == self.STEP:
            t = t.clone()
            t[..., 15] = t[..., 16]
        return t


class FusedColumnOff(SimDevice):
    """A fused bottleneck whose last column of every 16-wide tile is off by 16 ulps of T, with a random sign."""

    STEP = "hg.0.hg.3.0.0.conv3"

    def post(self, name, t):
        if name == self.STEP:
            t = t.clone()
            col = t[..., 15::16]
            sign = torch.where(torch.rand(col.shape, generator=torch.Generator().manual_seed(1)) < 0.5, -1.0, 1.0)
            t[..., 15::16] = col + sign * 16 * hl.ulp(col, self.storage).to(t.dtype)
        return t


class ChannelOffByFourUlp(SimDevice):
    """One output channel of a single-convolution step off by 4 ulps of T, with a random sign per element."""

    STEP = "res.0.0.conv2"

    def post(self, name, t):
        if name == self.STEP:
            t = t.clone()
            ch = t[:, 5]
            sign = torch.where(torch.rand(ch.shape, generator=torch.Generator().manual_seed(2)) < 0.5, -1.0, 1.0)
            t[:, 5] = ch + sign * 4 * hl.ulp(ch, self.storage).to(t.dtype)
        return t


class PreactWithoutRelu(SimDevice):
    """The pre-activation of one bottleneck without its ReLU on the first eight input channels."""

    BLOCK = "layer2.0"

    def preact(self, name, x):
        a = super().preact(name, x)
        if name == self.BLOCK:
            s, t = self.preact_st[name]
            a[:, :8] = self.rnd((x[:, :8].double() * s[None, :8, None, None].double() + t[None, :8, None, None].double()).float())
        return a


@pytest.fixture(scope="module")
def net():
    return oh.build(seed=0)


@pytest.fixture(scope="module")
def image():
    return torch.rand((1, 64, 64, 3), generator=torch.Generator().manual_seed(64), dtype=torch.float32)


def check_device(net, image, device_arith, fused=False):
    """Run a simulated device (every step stored, or the fused plan's steps), force the float64 oracle with its steps,
    return {step: violations} and the worst figures."""
    stored = fused_plan(oh.forward_traced(net, image)) if fused else _Every()
    dev = oh.forward_traced(net, image, arith=device_arith, steps=stored)
    dev = {k: v for k, v in dev.items() if k in stored}
    forced = {k: v for k, v in dev.items() if k != FINAL}
    A = oh.Arith(net, device_arith.storage)
    ref = oh.forward_traced(net, image, forced=forced, arith=A)
    bad, worst = {}, {}
    for name in dev:
        fam = "direct" if A.storage == "f32" else "fused" if name in A.fused else "unfused"
        fig = hl.figures(dev[name], ref[name], A.scale[name], A.storage, exact=name in A.exact, rounded=name != FINAL, fused=fam == "fused")
        v = hl.violations(fig, A.storage, fam)
        if v:
            bad[name] = v
        for k, x in fig.items():
            if k in ("err", "ulp", "mismatch") and x >= worst.get(k, (-1, None))[0]:
                worst[k] = (x, name)
            if k == "bias" and abs(x) >= abs(worst.get(k, (0, None))[0]):
                worst[k] = (x, name)
            if k == "equal" and x <= worst.get(k, (2, None))[0]:
                worst[k] = (x, name)
    return bad, worst


def test_forcing_with_the_oracles_own_trace_reproduces_it(net, image):
    own = oh.forward_traced(net, image)
    assert torch.equal(own[FINAL], oh.forward_nhwc(net, image))
    again = oh.forward_traced(net, image, forced={k: v for k, v in own.items() if k != FINAL})
    assert own.keys() == again.keys()
    for k in own:
        assert torch.equal(own[k], again[k]), k


def test_forced_step_is_one_layer_on_the_forced_inputs(net, image):
    """A forced tensor replaces the oracle's value for everything downstream: perturbing it moves the next step only
    through that step's own arithmetic."""
    own = oh.forward_traced(net, image)
    bumped = own["layer2.0.conv3"] + 1.0
    again = oh.forward_traced(net, image, forced={"layer2.0.conv3": bumped})
    assert torch.equal(again["layer2.0.conv3"], own["layer2.0.conv3"])   # the record is the oracle's own value
    assert torch.equal(again["layer1.0.conv3"], own["layer1.0.conv3"])
    assert not torch.equal(again["layer3.0.conv1"], own["layer3.0.conv1"])


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("storage", ["f32", "bf16", "f16"])
def test_simulated_device_passes(net, image, storage, fused):
    bad, worst = check_device(net, image, SimDevice(net, storage), fused=fused)
    print(f"simulated {storage} device ({'fused' if fused else 'unfused'} plan): worst {worst}")
    assert not bad, bad
    assert worst["mismatch"][0] == 0   # pools and up-adds bit-identical


MUTANTS = [("bf16", Truncating), ("f32", BiasDropped), ("bf16", BiasDropped), ("f16", BiasDropped), ("f32", BottomPadOffByOne),
           ("bf16", BottomPadOffByOne), ("f16", BottomPadOffByOne), ("f32", TileColumnFromNeighbour), ("bf16", TileColumnFromNeighbour),
           ("f16", TileColumnFromNeighbour), ("f16", PreactWithoutRelu), ("bf16", ChannelOffByFourUlp), ("f16", ChannelOffByFourUlp)]
# in the fused plan (t1 / t2 not stored: the fused steps' own bounds)
FUSED_MUTANTS = [("bf16", Truncating), ("bf16", FusedColumnOff), ("f16", FusedColumnOff), ("bf16", TileColumnFromNeighbour)]


@pytest.mark.parametrize("storage,mutant,fused", [m + (False,) for m in MUTANTS] + [m + (True,) for m in FUSED_MUTANTS],
                         ids=[f"{s}-{m.__name__}" for s, m in MUTANTS] + [f"fused-{s}-{m.__name__}" for s, m in FUSED_MUTANTS])
def test_mutant_is_detected(net, image, storage, mutant, fused):
    bad, _ = check_device(net, image, mutant(net, storage), fused=fused)
    assert bad, f"{mutant.__name__} ({storage}) passed the checker"
    first = next(iter(bad))
    print(f"{mutant.__name__} ({storage}) detected at {len(bad)} step(s), first {first}: {bad[first]}")
    target = getattr(mutant, "STEP", None) or getattr(mutant, "BLOCK", None)
    if target is not None:   # the wrong step itself is flagged (not only what consumes it)
        assert any(name.startswith(target) for name in bad), bad
    if mutant is Truncating:   # the mean signed error alone sees a biased conversion
        assert any("mean signed error" in v for vs in bad.values() for v in vs), bad
