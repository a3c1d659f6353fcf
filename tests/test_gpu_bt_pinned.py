"""The heat-maps of the engines whose bottlenecks stream their weights through the LDS-DMA ring, pinned bit for bit: those kernels share
their tile walk, t1 halo DMA, weight-ring issue and phase-2 lane set-up (csrc/hg_bt_common.h), and a slip in a shared piece must not pass
as a rounding difference.  The other hourglass tests compare with the oracle at a tolerance, or with the engine itself.

  * forward() of a 64 x 192 engine: at quarter resolution the bottleneck tiles (8 x 16 pixels) are 2 x 3 per view, at half resolution
    layer1's Winograd tiles (8 x 32) are 4 x 3 -- tiles_x != tiles_y, which a transposed tile decode cannot pass;
  * at V = 1 (6 quarter-resolution tiles: not a multiple of 8, and no workgroup of a persistent kernel has a next tile) and at a V that
    follows from the device's CU count (many_views): more quarter-resolution tiles than the largest persistent grid (2 per CU:
    conv1_ring_f32_kernel), no multiple of the Winograd grids (cu & ~7 workgroups), of 2 cu, or of 8 -- every persistent kernel ends on a
    partial round and the XCD map's eighths are unequal;
  * in the configurations of CONFIGS, which together launch every instantiation of the kernels that include hg_bt_common.h
    (test_every_touched_instantiation_is_launched checks the engines' profile names against TOUCHED):
        bottleneck_ring_kernel<T, UP, CIN, ADD2, MODE>      T in __hip_bfloat16, _Float16; MODE in 0, 1, 2;
                                                            (UP, CIN, ADD2) in (false, 256, false), (true, 256, false), (false, 256, true), (false, 128, false)
        bottleneck_l1_kernel<T>                             T in __hip_bfloat16, _Float16
        bottleneck_ring_f32_kernel<UP, ADD2, TAIL, T>       (UP, ADD2) in (false, false), (true, false), (false, true); TAIL in false, true; T in float, hgk::F32S
        conv1_ring_f32_kernel<UP, CIN, PL, T>               (UP, CIN, PL) in (false, 256, 128), (true, 256, 128), (false, 64, 64), (false, 128, 128); T in float, hgk::F32S
        conv1_res_f32_kernel
        layer1_tail_f32_kernel<T>, layer2_tail_f32_kernel<T>   T in float, hgk::F32S
        bottleneck_wino_f32_kernel<UP, ADD2, L2>            (false, false, false), (true, false, false), (false, true, false), (false, false, true)
        layer1_wino_f32_kernel
        head_kernel<T, LAST>                                T in float, hgk::F32S, __hip_bfloat16, _Float16; LAST in false, true
    None is left unpinned: every one of them can be reached through HourglassEngine's options.

The digests in tests/golden/hg_bt_digests.json were recorded with `python tests/test_gpu_bt_pinned.py` (on the GPU), twice in two
processes that agreed; "cu" is the compute-unit count of the device they were recorded on (the larger V follows from it)."""
import ctypes
import hashlib
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hg_bt_digests.json")
BT_H, BT_W = 64, 192
BT_TILES = (BT_H // 4 // 8) * (BT_W // 4 // 16)       # 2 x 3 tiles of 8 x 16 pixels per view at quarter resolution
# append only: a case's input seed is its position in CASES, so a configuration inserted or moved would change the inputs behind later digests
CONFIGS = [
    ("f32", {}),                                      # Winograd tails, conv1_res / conv1_ring
    ("f32", {"wino": 0}),                             # the TAIL form, layer1_tail_f32, layer2_tail_f32
    ("f32", {"wino": 0, "split1": 0}),                # the non-TAIL ring kernel
    ("f32s", {}),
    ("bf16", {}),                                     # ring MODE 2, bottleneck_l1_kernel
    ("f16", {}),
    ("bf16", {"w2d": 0}),                             # MODE 0
    ("f16", {"ring2": 0}),                            # MODE 1
    ("f32", {"fuse_upadd": 1}),                       # ADD2 and plain
    ("f32", {"fuse_upadd": 2}),                       # UP and plain
    ("f32", {"fuse_upadd": False}),                   # plain only
    ("bf16", {"fuse_upadd": 1}),
    ("bf16", {"fuse_upadd": 2}),
    ("bf16", {"fuse_upadd": False}),
    # the remaining (UP, type, MODE / TAIL) combinations
    ("f32", {"wino": 0, "fuse_upadd": 2}),
    ("f32", {"wino": 0, "split1": 0, "fuse_upadd": 2}),
    ("f32s", {"fuse_upadd": 2}),
    ("f32s", {"split1": 0}),
    ("f32s", {"split1": 0, "fuse_upadd": 2}),
    ("f16", {"fuse_upadd": 2}),
    ("bf16", {"w2d": 0, "fuse_upadd": 2}),
    ("f16", {"w2d": 0}),
    ("f16", {"w2d": 0, "fuse_upadd": 2}),
    ("bf16", {"ring2": 0}),
    ("bf16", {"ring2": 0, "fuse_upadd": 2}),
    ("f16", {"ring2": 0, "fuse_upadd": 2}),
]
CASES = [(c, v) for c in range(len(CONFIGS)) for v in ("one", "many")]

_B = ("false", "true")
_F32T, _LPT = ("float", "hgk::F32S"), ("__hip_bfloat16", "_Float16")
TOUCHED = sorted(
    [f"bottleneck_ring_kernel<{t}, {up}, {cin}, {add2}, {mode}>" for t in _LPT for mode in (0, 1, 2)
     for up, cin, add2 in (("false", 256, "false"), ("true", 256, "false"), ("false", 256, "true"), ("false", 128, "false"))]
    + [f"bottleneck_l1_kernel<{t}>" for t in _LPT]
    + [f"bottleneck_ring_f32_kernel<{up}, {add2}, {tail}, {t}>" for up, add2 in (("false", "false"), ("true", "false"), ("false", "true")) for tail in _B for t in _F32T]
    + [f"conv1_ring_f32_kernel<{up}, {cin}, {pl}, {t}>" for up, cin, pl in (("false", 256, 128), ("true", 256, 128), ("false", 64, 64), ("false", 128, 128)) for t in _F32T]
    + ["conv1_res_f32_kernel", "layer1_wino_f32_kernel"]
    + [f"{k}<{t}>" for k in ("layer1_tail_f32_kernel", "layer2_tail_f32_kernel") for t in _F32T]
    + [f"bottleneck_wino_f32_kernel<{a}>" for a in ("false, false, false", "true, false, false", "false, true, false", "false, false, true")]
    + [f"head_kernel<{t}, {last}>" for t in _F32T + _LPT for last in _B])
TOUCHED_KERNELS = sorted({n.split("<")[0] for n in TOUCHED})


def config_name(i):
    dtype, opts = CONFIGS[i]
    return " ".join([dtype] + [f"{k}={int(v)}" for k, v in opts.items()])


def case_name(c):
    return f"{config_name(c[0])} {c[1]}"


def many_views(cu):
    return 2 * cu // BT_TILES + 4   # 256 CUs: 89 views, 534 tiles


def many_ok(tiles, cu):
    return tiles > 2 * cu and tiles % (cu & ~7) != 0 and tiles % (2 * cu) != 0 and tiles % 8 != 0


def engine(i, engines, device):
    from deepfly3d_amd.hourglass import HourglassEngine
    from deepfly3d_amd.synthetic import synthetic_state_dict

    if i not in engines:
        dtype, opts = CONFIGS[i]
        engines[i] = HourglassEngine(synthetic_state_dict(3), dtype=dtype, device=device, height=BT_H, width=BT_W, **opts)
    return engines[i]


def digest(case, engines, device, cu):
    """engines: index into CONFIGS -> HourglassEngine, filled here"""
    import torch

    views = 1 if case[1] == "one" else many_views(cu)
    if case[1] == "many":
        assert many_ok(views * BT_TILES, cu), (views, cu)
    g = torch.Generator().manual_seed(40 + CASES.index(case))
    images = torch.rand((views, BT_H, BT_W, 3), generator=g) * 2.0 - 0.75
    hm = engine(case[0], engines, device).forward(images.to(device))
    return hashlib.sha256(hm.cpu().numpy().tobytes()).hexdigest()


def launched(eng, device):
    """profile names of the kernels one forward() of a single view launches"""
    import torch

    from deepfly3d_amd import _native

    lib = eng.lib
    _native.check(lib.df3d_hg_profile(eng.h, 1))
    eng.forward(torch.zeros((1, BT_H, BT_W, 3), device=device))
    torch.cuda.synchronize()
    names = set()
    buf = ctypes.create_string_buffer(128)
    for k in range(lib.df3d_hg_profile_count(eng.h)):
        ms, fl, by, m1, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _native.check(lib.df3d_hg_profile_read(eng.h, k, buf, 128, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(m1), ctypes.byref(n)))
        if n.value:
            names.add(buf.value.decode())
    _native.check(lib.df3d_hg_profile(eng.h, 0))
    return names


@pytest.fixture(scope="module")
def engines():
    return {}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    omitted = fx["omitted"]
    # a case that did not repeat at the commit the digests were recorded at may be left out: one at most, and none of the default configurations
    defaults = {case_name((i, v)) for i in range(len(CONFIGS)) if not CONFIGS[i][1] for v in ("one", "many")}
    assert len(omitted) <= 1 and not defaults & set(omitted), omitted
    assert sorted(list(fx["digests"]) + omitted) == sorted(case_name(c) for c in CASES)
    return fx


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_bottleneck_output_is_unchanged(cuda, engines, recorded, case):
    import torch

    name = case_name(case)
    if name in recorded["omitted"]:
        pytest.skip(f"{name}: not reproducible where the digests were recorded")
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    if case[1] == "many" and cu != recorded["cu"]:
        pytest.skip(f"{name}: the view count follows from the CU count; recorded on {recorded['cu']} CUs, this device has {cu}")
    got = digest(case, engines, cuda, cu)
    assert got == recorded["digests"][name], f"{name}: the output changed"


@pytest.mark.gpu
def test_every_touched_instantiation_is_launched(cuda, engines):
    seen = set()
    for i in range(len(CONFIGS)):
        seen |= launched(engine(i, engines, cuda), cuda)
    ours = sorted(n for n in seen if n.split("<")[0] in TOUCHED_KERNELS)
    assert ours == TOUCHED, (sorted(set(TOUCHED) - seen), sorted(set(ours) - set(TOUCHED)))


if __name__ == "__main__":
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    engines = {}
    fx = {"cu": cu, "omitted": [], "digests": {case_name(c): digest(c, engines, dev, cu) for c in CASES}}
    with open(out, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print(json.dumps(fx, indent=1))
    seen = set()
    for i in range(len(CONFIGS)):
        seen |= launched(engine(i, engines, dev), dev)
    print("launched:", json.dumps(sorted(seen), indent=1))
    print("touched but not launched:", sorted(set(TOUCHED) - seen))
    print("launched, of a touched kernel, not listed:", sorted(n for n in seen if n.split("<")[0] in TOUCHED_KERNELS and n not in TOUCHED))
