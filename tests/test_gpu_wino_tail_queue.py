"""The fp32 Winograd tails' vector-memory queue (csrc/hg_bt_wino_f32.h): the kernels keep residual loads, LDS-DMA pieces of the next tile's halo,
W3 ring stages and output stores in flight together and tell them apart by COUNTED waits (operations retire in issue order).  A miscounted
wait is a timing-dependent error -- a value read before it landed -- so every case runs FIVE times on a NaN-poisoned workspace and must repeat
bit for bit, on top of the comparison of every plan step with the `wino=0` engine at the fp32 engine's tolerance (5e-5 of the step's range,
tests/test_gpu_hourglass.py FP32_TOL).  The pinned digests (test_gpu_bt_pinned.py, test_gpu_wino_steps_pinned.py) hold the values themselves.

Sizes
  * one view of 64 x 128: the 16 x 32 level is 2 x 2 tiles, the 8 x 16 level one tile -- every workgroup walks exactly one tile: the first tile
    is the last, and no halo is requested for a next one;
  * 128 x 256 with 2 cu / 16 + 1 views (cu: the device's compute-unit count; 33 views, 528 tiles on 256 CUs): the 32 x 64 level has more than
    2 cu tiles, no multiple of the persistent grid (cu & ~7) or of 2 cu, so workgroups walk 2 and 3 tiles -- the metered halo requests and the
    path without a next tile both run.  (test_gpu_bt_pinned.many_ok also asks for a tile count that is no multiple of 8; at 16 tiles per
    view that cannot hold and is not asked here.)

Engines: the default fp32 engine (the producer-side up-path sum: plain, ADD2 and layer2 tails) and `fuse_upadd=2` (the consumer-side sum: the UP
tail, which the default plan does not contain); test_all_four_instantiations_and_pooled_forms_are_launched reads the launch log step by step.
Pooled forms (df3d_hg_step_pooled: the 2x2 max-pooled tensors a block writes beside its output, which change the number of stores the wait in
front of the second output half has to let pass): blocks with a pooled output, with a pooled input and with neither are in these plans.  A block
with BOTH does not occur in any plan of the engine: the pooled input is asked for by the first block of an hourglass level's low branch, of which
nobody pools the output (hg_plan.h), so that form of the wait is reached by no launch and is not invented here."""
import ctypes

import pytest

FP32_TOL = 5e-5
REPEATS = 5
SIZES = {"one": (64, 128), "many": (128, 256)}
OPTIONS = [{}, {"fuse_upadd": 2}]
CASES = [(o, s) for o in range(len(OPTIONS)) for s in SIZES]
WINO_TAILS = sorted(f"bottleneck_wino_f32_kernel<{a}>" for a in ("false, false, false", "true, false, false", "false, true, false", "false, false, true"))


def case_name(c):
    return " ".join(["f32"] + [f"{k}={int(v)}" for k, v in OPTIONS[c[0]].items()] + [c[1]])


def views_of(size, cu):
    return 1 if size == "one" else 2 * cu // 16 + 1


def engine(engines, device, opt, size, wino):
    from deepfly3d_amd.hourglass import HourglassEngine
    from deepfly3d_amd.synthetic import synthetic_state_dict

    key = (opt, size, wino)
    if key not in engines:
        h, w = SIZES[size]
        engines[key] = HourglassEngine(synthetic_state_dict(3), dtype="f32", device=device, height=h, width=w, wino=wino, **OPTIONS[opt])
    return engines[key]


@pytest.fixture(scope="module")
def engines():
    return {}


def steps_on_poison(eng, images):
    """the output tensor of every plan step, each from a forward on a workspace of NaNs"""
    out = []
    for k in range(1, len(eng.steps()) + 1):
        eng._workspace(images.shape[0]).fill_(0xFF)
        out.append(eng.forward_upto(images, k))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_every_step_repeats_bit_for_bit_and_matches_the_direct_tails(cuda, engines, case):
    import torch

    opt, size = case
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    views = views_of(size, cu)
    h, w = SIZES[size]
    if size == "many":
        tiles, grid = views * (h // 4 // 8) * (w // 4 // 16), cu & ~7
        assert tiles > 2 * cu and tiles % grid != 0 and tiles % (2 * cu) != 0, (tiles, cu)
    on, off = engine(engines, cuda, opt, size, 1), engine(engines, cuda, opt, size, 0)
    names = [n for n, _ in on.steps()]
    assert names == [n for n, _ in off.steps()]
    g = torch.Generator().manual_seed(9100 + CASES.index(case))
    images = (torch.rand((views, h, w, 3), generator=g) * 2.0 - 0.75).to(cuda)
    ref = steps_on_poison(off, images)
    first = steps_on_poison(on, images)
    for k, (name, a, b) in enumerate(zip(names, first, ref), start=1):
        assert bool(torch.isfinite(a).all()), f"step {k} {name}: a value that no kernel of this forward wrote"
        err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        assert err < FP32_TOL, f"step {k} {name}: rel err {err:.3e} against the wino=0 engine"
    for run in range(1, REPEATS):
        again = steps_on_poison(on, images)
        moved = [f"{k} {name}" for k, (name, a, b) in enumerate(zip(names, first, again), start=1) if not torch.equal(a, b)]
        assert not moved, f"run {run}: the output of step(s) {moved} differs from run 0 (the first one is where to look)"


def launched(eng, device, size, upto=None):
    """profile name -> number of launches of one forward() (upto None) or forward_upto(upto) of a single view"""
    import torch

    from deepfly3d_amd import _native

    lib = eng.lib
    _native.check(lib.df3d_hg_profile(eng.h, 1))
    images = torch.zeros((1, *SIZES[size], 3), device=device)
    if upto is None:
        eng.forward(images)
    else:
        eng.forward_upto(images, upto)
    torch.cuda.synchronize()
    counts = {}
    buf = ctypes.create_string_buffer(128)
    for k in range(lib.df3d_hg_profile_count(eng.h)):
        ms, fl, by, m1, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _native.check(lib.df3d_hg_profile_read(eng.h, k, buf, 128, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(m1), ctypes.byref(n)))
        if n.value:
            counts[buf.value.decode()] = n.value
    _native.check(lib.df3d_hg_profile(eng.h, 0))
    return counts


def wino_launches(counts):
    return {n: c for n, c in counts.items() if n.startswith("bottleneck_wino_f32_kernel")}


@pytest.mark.gpu
def test_all_four_instantiations_and_pooled_forms_are_launched(cuda, engines):
    """The launch log, step by step: the Winograd tails that forward_upto(k) launches and forward_upto(k - 1) does not are plan step k's own, and
    df3d_hg_step_pooled names the pooled tensors that step writes -- no guess from a step's name or shape at which kernel runs it."""
    for size in SIZES:
        seen, pooled = set(), set()
        for opt in range(len(OPTIONS)):
            eng = engine(engines, cuda, opt, size, 1)
            whole = wino_launches(launched(eng, cuda, size))
            before, total = {}, 0
            for k in range(1, len(eng.steps()) + 1):
                now = wino_launches(launched(eng, cuda, size, upto=k))
                own = {n for n in now if now[n] > before.get(n, 0)}
                before = now
                if own:
                    assert len(own) == 1, (size, k, own)
                    total += 1
                    seen |= own
                    form = eng.lib.df3d_hg_step_pooled(eng.h, k - 1)
                    assert form >= 0, (size, k)
                    pooled.add(form)
            assert total == sum(whole.values()) and before == whole, (size, whole, before)   # every tail launch of a forward() was seen at its step
        assert sorted(seen) == WINO_TAILS, (size, sorted(seen))
        # 0: neither, 1: the pooled output, 2: the pooled input; 3 (both) is in no plan of the engine (module docstring)
        assert pooled == {0, 1, 2}, (size, pooled)
