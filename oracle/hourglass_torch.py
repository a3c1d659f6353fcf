"""CPU oracle for the 2-D half of the hot path: stacked-hourglass forward in torch (fp32, NCHW).
TEST INFRASTRUCTURE ONLY -- the product package never imports this file.

PARITY UNPINNED for the network itself: the reference delegates the model to the un-vendored
`nely-df2d >= 0.14` (reference setup.py:31; call site df3d/core.py:177-185) and the trained
weights `sh8_deepfly.tar` (path only, reference df3d/config.py:30-32) are not in the checkout, so
no golden vector of the reference can exercise it here.  What the reference itself pins and this
file follows: 2 stacks (df3d/config.py:33), 19 output maps (df3d/config.py:36), 64x128 heat-maps
(df3d/config.py:18) from 256x512 inputs, hard arg-max + peak value (README.md:404).  The layer
structure is the published stacked-hourglass of Newell et al. in its pre-activation-bottleneck
PyTorch form that df2d uses: state_dict keys are kept compatible
(`conv1, bn1, layer{1,2,3}.0.*, hg.{s}.hg.{lvl}.{k}.0.*, res.{s}.0.*, fc.{s}.{0,1}, score.{s},
fc_.{s}, score_.{s}`) so trained weights can be loaded when a user has them.

The HIP engine is compared against this module layer by layer with seeded random parameters.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

NUM_CLASSES = 19
NUM_STACKS = 2
FEATS = 128  # bottleneck planes; trunk width = 2 * FEATS
DEPTH = 4


class PreActBottleneck(nn.Module):
    """x -> conv1x1(relu(bn1 x)) -> conv3x3(relu(bn2 .)) -> conv1x1(relu(bn3 .)) + skip(x)."""

    def __init__(self, cin, planes):
        super().__init__()
        cout = 2 * planes
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, planes, 1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1)
        self.bn3 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, cout, 1)
        self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1)) if cin != cout else None

    def forward(self, x):
        t = self.conv1(F.relu(self.bn1(x)))
        t = self.conv2(F.relu(self.bn2(t)))
        t = self.conv3(F.relu(self.bn3(t)))
        return t + (x if self.downsample is None else self.downsample(x))


def _unit(cin, planes):
    return nn.Sequential(PreActBottleneck(cin, planes))


class Hourglass(nn.Module):
    def __init__(self, planes=FEATS, depth=DEPTH):
        super().__init__()
        self.depth = depth
        levels = []
        for lvl in range(depth):  # lvl 0 is the innermost (lowest-resolution) level
            n = 4 if lvl == 0 else 3
            levels.append(nn.ModuleList([_unit(2 * planes, planes) for _ in range(n)]))
        self.hg = nn.ModuleList(levels)

    def _level(self, n, x):
        blocks = self.hg[n - 1]
        up1 = blocks[0](x)
        low = blocks[1](F.max_pool2d(x, 2, stride=2))
        low = self._level(n - 1, low) if n > 1 else blocks[3](low)
        low = blocks[2](low)
        return up1 + F.interpolate(low, scale_factor=2, mode="nearest")

    def forward(self, x):
        return self._level(self.depth, x)


class HourglassNet(nn.Module):
    def __init__(self, num_stacks=NUM_STACKS, num_classes=NUM_CLASSES, feats=FEATS):
        super().__init__()
        self.num_stacks = num_stacks
        ch = 2 * feats
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = _unit(64, 64)
        self.layer2 = _unit(128, feats)
        self.layer3 = _unit(ch, feats)
        self.hg = nn.ModuleList([Hourglass(feats) for _ in range(num_stacks)])
        self.res = nn.ModuleList([_unit(ch, feats) for _ in range(num_stacks)])
        self.fc = nn.ModuleList([nn.Sequential(nn.Conv2d(ch, ch, 1), nn.BatchNorm2d(ch)) for _ in range(num_stacks)])
        self.score = nn.ModuleList([nn.Conv2d(ch, num_classes, 1) for _ in range(num_stacks)])
        self.fc_ = nn.ModuleList([nn.Conv2d(ch, ch, 1) for _ in range(num_stacks - 1)])
        self.score_ = nn.ModuleList([nn.Conv2d(num_classes, ch, 1) for _ in range(num_stacks - 1)])

    def stem(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.max_pool2d(self.layer1(x), 2, stride=2)
        return self.layer3(self.layer2(x))

    def forward(self, x, return_all=False):
        outs = []
        x = self.stem(x)
        for s in range(self.num_stacks):
            y = self.res[s](self.hg[s](x))
            y = F.relu(self.fc[s](y))
            score = self.score[s](y)
            outs.append(score)
            if s < self.num_stacks - 1:
                x = x + self.fc_[s](y) + self.score_[s](score)
        return outs if return_all else outs[-1]


def seeded_state_dict(seed=0, num_stacks=NUM_STACKS, gain=0.6):
    """Seeded synthetic parameters: He-normal conv weights, small biases,
    BN gamma~U[0.5,1.5], beta,mean~N(0,0.1), var~U[0.5,1.5].  `gain` (0.6) scales the He std so
    the final heat-maps of the 2-stack net stay O(10).  Returns {name: float32 tensor}."""
    net = HourglassNet(num_stacks=num_stacks)
    g = torch.Generator().manual_seed(seed)
    sd = net.state_dict()
    out = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            out[k] = v.clone()
            continue
        if v.ndim == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            # residual branches are damped so 30+ stacked residual adds stay O(1)
            scale = (2.0 / fan_in) ** 0.5 * (gain if not k.endswith("conv3.weight") else 0.5 * gain)
            out[k] = torch.randn(v.shape, generator=g) * scale
        elif k.endswith("running_var") or (k.endswith("weight") and v.ndim == 1):
            out[k] = torch.rand(v.shape, generator=g) + 0.5
        else:  # conv bias, bn bias, running_mean
            out[k] = torch.randn(v.shape, generator=g) * 0.1
    return out


def build(seed=0, num_stacks=NUM_STACKS):
    net = HourglassNet(num_stacks=num_stacks)
    net.load_state_dict(seeded_state_dict(seed, num_stacks))
    net.eval()
    return net


@torch.no_grad()
def forward_nhwc(net, images_nhwc):
    """images_nhwc: (N, 256, 512, 3) float32 -> heat-maps (N, 19, 64, 128) float32."""
    x = torch.as_tensor(images_nhwc, dtype=torch.float32).permute(0, 3, 1, 2).contiguous()
    return net(x)


# ------------------------------------------------------------------------------------------------
# traced forward: the same arithmetic as HourglassNet.forward, recording every intermediate under the
# name of the engine plan step that produces it (deepfly3d_amd/csrc/hourglass.hip), NHWC float32.
# A convolution followed by BN(+ReLU) is recorded AFTER that BN/ReLU because the engine folds them.
#
# Teacher forcing (tests/test_gpu_hourglass_local.py): `forced` maps step names to NHWC tensors -- a device's own
# outputs.  At every step the oracle records ITS value and then continues from the forced tensor where there is
# one, so a step's record is that one layer evaluated on the device's inputs and its error is the error of one
# kernel.  A step the engine does not materialise (the inner convolutions of a fused bottleneck, layer1's
# full-resolution output when only its pooled copy is written) is not forced and keeps the oracle's value.
#
# `arith` (an Arith) replaces torch's modules by the engine's parameters and arithmetic: float64 (or float32)
# evaluation, and for the 16-bit engines the operand-rounding model.  It also records, per step, an
# element-wise magnitude scale (the same layer on absolute values), which steps are exact (no product) and which
# convolutions had an operand the device did not store (the step is then a fused kernel with roundings inside).
# ------------------------------------------------------------------------------------------------
BN_EPS = 1e-5
STORAGE_BITS = {"f32": 24, "bf16": 8, "f16": 11}   # significand bits (with the implicit one)
_TORCH_STORAGE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def round_to(t, storage):
    """Round to the storage format, nearest-even, through float32 (what the device's converters see)."""
    return t.to(torch.float32).to(_TORCH_STORAGE[storage]).to(t.dtype)


def _folded(net):
    """{conv name: (weight, bias)} as the engine stores them: the following BatchNorm folded in float64, the result
    kept as float32 (deepfly3d_amd/hourglass.py pack_state_dict), and {bottleneck: (scale, shift)} of each input BN."""
    def bn(m):
        s = m.weight.double() / torch.sqrt(m.running_var.double() + BN_EPS)
        return s, m.bias.double() - m.running_mean.double() * s

    def fold(conv, m=None):
        w, b = conv.weight.double(), conv.bias.double()
        if m is not None:
            s, t = bn(m)
            w, b = w * s[:, None, None, None], b * s + t
        return w.float().double(), b.float().double()

    convs, preact = {"conv1": fold(net.conv1, net.bn1)}, {}

    def block(name, seq):
        b = seq[0]
        convs[name + ".conv1"] = fold(b.conv1, b.bn2)
        convs[name + ".conv2"] = fold(b.conv2, b.bn3)
        convs[name + ".conv3"] = fold(b.conv3)
        if b.downsample is not None:
            convs[name + ".downsample.0"] = fold(b.downsample[0])
        s, t = bn(b.bn1)
        preact[name] = (s.float().double(), t.float().double())

    for name in ("layer1", "layer2", "layer3"):
        block(name + ".0", getattr(net, name))
    for s in range(net.num_stacks):
        for lvl, blocks in enumerate(net.hg[s].hg):
            for k, seq in enumerate(blocks):
                block(f"hg.{s}.hg.{lvl}.{k}.0", seq)
        block(f"res.{s}.0", net.res[s])
        convs[f"fc.{s}.0"] = fold(net.fc[s][0], net.fc[s][1])
        convs[f"score.{s}"] = fold(net.score[s])
        if s < net.num_stacks - 1:
            convs[f"fc_.{s}"] = fold(net.fc_[s])
            convs[f"score_.{s}"] = fold(net.score_[s])
    return convs, preact


class Arith:
    """The engine's arithmetic for forward_traced: parameters as the engine stores them, evaluated in `dtype`.

    storage "f32" (the f32 / f32s engines): no rounding inside a convolution; pools and up-adds round to float32.
    storage "bf16" / "f16": the operand-rounding model of deepfly3d_amd/csrc/hg_types.h -- conversions are
    round-to-nearest-even (hg_types.h:27, Lp<T>::from_f32 / pack2), the pre-activation is fmaxf(fmaf(x, s, t), 0)
    rounded to T (hg_types.h:124-133; hg_bt_reg.h:186 for the up-add input), weights are the float32 blob
    rounded to T (hg_pool.h:122), the stem's image patch is rounded to T (stem_lp_kernel, hg_stem.h),
    accumulation is exact here (fp32 on the device), and a single-convolution step stores round_T(accumulator + bias (+ residual)).
    Roundings inside fused kernels, made at the same points:
      * bottleneck kernels (hg_bt_reg.h bottleneck_kernel, hg_bt_ring.h, hg_bt_l1.h): t1 and t2 are T operands of the next
        GEMM (rounded); the downsample is summed into conv3's accumulator (hg_bt_reg.h:311-319, bias b3 + bd) and NOT
        rounded on its own; with an identity skip the output is round_T(round_T(accumulator + bias) + x) (hg_bt_ring.h:710-723,
        hg_bt_reg.h:512-529: the accumulator is packed to T, then add_chunk adds the residual and rounds again);
      * ADD2 epilogue (fuse_upadd=1): the rounded block output + the low-resolution tensor, rounded again (hg_bt_reg.h:531);
      * head_kernel (hg_head.h:317, 430): y and score are rounded to T as operands; x_new = round_T(x + fc_(y) + score_(score))
        from ONE accumulator (hg_head.h:505-517), so fc_'s sum is not rounded when it is not a step of its own;
      * the final heat-maps are float32 planes: score of the last stack is never rounded to T.
    After forward_traced: `scale[name]` (NHWC float64), `exact` (the names of steps with no product, whose inputs
    were all forced) and `fused` (convolutions with an operand that was not forced) describe each recorded step."""

    def __init__(self, net, storage="f32", dtype=torch.float64):
        self.storage, self.dtype = storage, dtype
        convs, preact = _folded(net)
        lp = storage != "f32"
        self.w = {k: (round_to(w, storage) if lp else w).to(dtype) for k, (w, b) in convs.items()}
        self.b = {k: b.to(dtype) for k, (w, b) in convs.items()}
        self.preact_st = {k: (s.to(dtype), t.to(dtype)) for k, (s, t) in preact.items()}
        self.scale, self.exact, self.fused = {}, set(), set()

    # --- overridable pieces (tests/test_oracle_forced.py builds simulated devices and their mutants from them) ---
    def rnd(self, t):
        return round_to(t, self.storage) if self.storage != "f32" else t

    def rnd_sum(self, t):   # pools / up-adds: stored in the storage format, float32 included
        return round_to(t, self.storage)

    def conv(self, name, a, stride, pad):
        return F.conv2d(a, self.w[name], self.b[name], stride=stride, padding=pad)

    def preact(self, name, x):
        s, t = self.preact_st[name]
        a = x * s[None, :, None, None] + t[None, :, None, None]
        if self.storage != "f32":
            a = self.rnd(a.float().to(self.dtype))   # fmaf in float32, then the conversion to T
        return a.clamp_min(0)

    def post(self, name, t):   # a step's value as stored (a hook for mutants)
        return t


@torch.no_grad()
def forward_traced(net, images_nhwc, forced=None, arith=None, steps=None):
    """Every plan step's output, NHWC (the final heat-maps NCHW).  `forced` / `arith`: see the block comment above;
    with neither the result is HourglassNet.forward's fp32 arithmetic, step by step.  `steps` (default: the forced
    names): the steps the device stores, which decides where the 16-bit model rounds a sum a fused kernel keeps."""
    rec = {}
    forced = forced or {}
    stored = set(forced) if steps is None else steps
    A = arith
    dt = A.dtype if A is not None else torch.float32

    def nhwc(t):
        return t.permute(0, 2, 3, 1).contiguous()

    # a tensor is (value NCHW, scale NCHW or None, exact: computed without a product from forced tensors only)
    def keep(name, v):
        t, s, ex = v
        if A is not None:
            t = A.post(name, t)
            A.scale[name] = nhwc(s)
            if ex:
                A.exact.add(name)
        rec[name] = nhwc(t)
        if name in forced:
            f = torch.as_tensor(forced[name]).to(dt).permute(0, 3, 1, 2).contiguous()
            return f, (f.abs() if A is not None else None), True
        return t, s, ex

    def layer(name, a, stride=1, pad=0, relu=False, skip=None, skip_in_acc=False, round_before_skip=False, rnd=True, inputs=()):
        """conv `name` on the operand a (already pre-activated / rounded), + skip, ReLU, stored; `inputs`: the tensors it reads.
        The scale is the layer on the magnitudes of the operands it actually reads: conv(|a|, |w|) + |b| + |skip| (a skip
        summed in the same accumulator -- the fused downsample -- contributes its own such scale)."""
        if not all(v[2] for v in inputs):
            A.fused.add(name)
        y = A.conv(name, a, stride, pad)
        s = F.conv2d(a.abs(), A.w[name].abs(), A.b[name].abs(), stride=stride, padding=pad)
        if skip is not None:
            if round_before_skip:
                y = A.rnd(y)
            y, s = y + skip[0], s + (skip[1] if skip_in_acc else skip[0].abs())
        if relu:
            y = y.clamp_min(0)
        return (A.rnd(y) if rnd else y), s, False

    def operand(v):   # a tensor entering a GEMM: the device's T copy of it
        return A.rnd(v[0])

    def block(name, seq, x):
        b = seq[0]
        if A is None:
            t = keep(name + ".conv1", (F.relu(b.bn2(b.conv1(F.relu(b.bn1(x[0]))))), None, False))
            t = keep(name + ".conv2", (F.relu(b.bn3(b.conv2(t[0]))), None, False))
            skip = x if b.downsample is None else keep(name + ".downsample.0", (b.downsample(x[0]), None, False))
            return keep(name + ".conv3", (b.conv3(t[0]) + skip[0], None, False))
        a = A.preact(name, x[0])
        t = keep(name + ".conv1", layer(name + ".conv1", a, relu=True, inputs=(x,)))
        t = keep(name + ".conv2", layer(name + ".conv2", operand(t), pad=1, relu=True, inputs=(t,)))
        ds = name + ".downsample.0"
        if b.downsample is None:
            skip = x
        else:   # fused: summed into conv3's accumulator unrounded; unfused: a stored step, forced
            skip = keep(ds, layer(ds, operand(x), rnd=ds in stored, inputs=(x,)))
        # the fused bottleneck with an identity skip rounds conv3's accumulator (bias included) to T, then adds the skip and
        # rounds again: hg_bt_ring.h:710-723 and hg_bt_reg.h:512-529 (Lp<T>::pack2 into the epilogue slice, then add_chunk);
        # the single-convolution kernel adds the residual to the accumulator (one rounding)
        twice = A.storage != "f32" and b.downsample is None and name + ".conv2" not in stored
        return keep(name + ".conv3", layer(name + ".conv3", operand(t), skip=skip, skip_in_acc=ds not in stored, round_before_skip=twice,
                                           inputs=(t, skip)))

    def pool(x):
        if A is None:
            return F.max_pool2d(x[0], 2, stride=2), None, False
        v = F.max_pool2d(x[0], 2, stride=2)
        return (A.rnd_sum(v) if x[2] else A.rnd(v)), F.max_pool2d(x[1], 2, stride=2), x[2]

    def upadd(hi, lo):
        up = F.interpolate(lo[0], scale_factor=2, mode="nearest")
        if A is None:
            return hi[0] + up, None, False
        ex = hi[2] and lo[2]   # (not exact: the ADD2 epilogue's sum, rounded again -- or, in float32 storage, not at all)
        return (A.rnd_sum(hi[0] + up) if ex else A.rnd(hi[0] + up)), hi[1] + F.interpolate(lo[1], scale_factor=2, mode="nearest"), ex

    def level(prefix, hg, n, x):
        lv = f"{prefix}.{n - 1}"
        blocks = hg.hg[n - 1]
        up1 = block(lv + ".0.0", blocks[0], x)
        low = keep(lv + ".pool", pool(x))
        low = block(lv + ".1.0", blocks[1], low)
        low = level(prefix, hg, n - 1, low) if n > 1 else block(lv + ".3.0", blocks[3], low)
        low = block(lv + ".2.0", blocks[2], low)
        return keep(lv + ".upadd", upadd(up1, low))

    x = torch.as_tensor(images_nhwc, dtype=torch.float32).permute(0, 3, 1, 2).contiguous()
    if A is None:
        x = keep("conv1", (F.relu(net.bn1(net.conv1(x))), None, False))
    else:
        x = keep("conv1", layer("conv1", A.rnd(x.to(dt)), stride=2, pad=3, relu=True))
    x = block("layer1.0", net.layer1, x)
    x = keep("maxpool", pool(x))
    x = block("layer2.0", net.layer2, x)
    x = block("layer3.0", net.layer3, x)
    for s in range(net.num_stacks):
        last = s == net.num_stacks - 1
        y = level(f"hg.{s}.hg", net.hg[s], net.hg[s].depth, x)
        y = block(f"res.{s}.0", net.res[s], y)
        if A is None:
            y = keep(f"fc.{s}.0", (F.relu(net.fc[s](y[0])), None, False))
            score = (net.score[s](y[0]), None, False)
        else:
            y = keep(f"fc.{s}.0", layer(f"fc.{s}.0", operand(y), relu=True, inputs=(y,)))
            score = layer(f"score.{s}", operand(y), rnd=not last, inputs=(y,))
        if not last:
            score = keep(f"score.{s}", score)
            if A is None:
                t = keep(f"fc_.{s}", (x[0] + net.fc_[s](y[0]), None, False))
                x = keep(f"score_.{s}", (t[0] + net.score_[s](score[0]), None, False))
            else:   # fused head: one accumulator, fc_'s sum unrounded unless it is a step of its own
                t = keep(f"fc_.{s}", layer(f"fc_.{s}", operand(y), skip=x, rnd=f"fc_.{s}" in stored, inputs=(y, x)))
                x = keep(f"score_.{s}", layer(f"score_.{s}", operand(score), skip=t, skip_in_acc=f"fc_.{s}" not in stored, inputs=(score, t)))
        else:
            rec[f"score.{s}"] = score[0].contiguous()  # the final heat-maps stay NCHW
            if A is not None:
                A.scale[f"score.{s}"] = score[1].contiguous()
    return rec
