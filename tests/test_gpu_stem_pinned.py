"""The three stem kernels' outputs, pinned bit for bit: the stems share their tile decode, patch gather (with the front-end's
df3d_pre::pixel sampling behind df3d_hg_forward_u8), weight copy and fp32 epilogue (csrc/hg_stem.h), and a slip in a shared piece
must not pass as a rounding difference.  The other stem tests compare with the oracle at a tolerance, or with the engine itself.

  * stem output (forward_upto(images, 1)) of a 64 x 192 engine, 4 x 6 tiles per view -- tiles_x != tiles_y, which a square tile grid
    would not tell apart -- at V = 1 (no workgroup has a next tile) and at V = 4 cu // 24 + 3 (more tiles than the largest stem grid,
    4 per CU, and no whole number of rounds of any of the three grids: every stem prefetches a next tile behind its K loop, scatters
    it between the barriers, and ends on a partial round);
  * heat-maps of forward_u8 on the default 256 x 512 engine at V = 5 (1 280 tiles: the u8 sampling path on a next-tile prefetch in
    every engine), from grey and from 3-channel frames, with flips and a non-trivial mean / std.

The digests in tests/golden/hg_stem_digests.json were recorded with `python tests/test_gpu_stem_pinned.py` (on the GPU), twice in two
processes that agreed; "cu" is the compute-unit count of the device they were recorded on (the larger V follows from it)."""
import hashlib
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hg_stem_digests.json")
DTYPES = ("f32", "bf16", "f16", "f32s")
STEM_H, STEM_W = 64, 192                       # 4 x 6 tiles of 8 x 16 output pixels per view
STEM_TILES = (STEM_H // 2 // 8) * (STEM_W // 2 // 16)
U8_FRAMES = {"grey": (5, 120, 200), "rgb": (5, 301, 517, 3)}
U8_FLIP = [0, 1, 0, 1, 1]
U8_MEAN, U8_STD = (0.22, 0.31, 0.18), (0.9, 1.1, 1.3)
# append only: a case's input seed is its position in this list, so a case inserted or moved would change the inputs behind later digests
CASES = [("stem", d, v) for d in DTYPES for v in ("one", "many")] + [("u8", d, f) for d in DTYPES for f in U8_FRAMES]


def case_name(c):
    return " ".join(c)


def many_views(cu):
    return 4 * cu // STEM_TILES + 3


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def digest(case, engines, device, cu):
    """engines: (dtype, height, width) -> HourglassEngine, filled here"""
    import torch

    from deepfly3d_amd.hourglass import HourglassEngine
    from deepfly3d_amd.synthetic import synthetic_state_dict

    kind, dtype, which = case
    hw = (STEM_H, STEM_W) if kind == "stem" else (256, 512)
    if (dtype, *hw) not in engines:
        engines[(dtype, *hw)] = HourglassEngine(synthetic_state_dict(3), dtype=dtype, device=device, height=hw[0], width=hw[1])
    eng = engines[(dtype, *hw)]
    g = torch.Generator().manual_seed(20 + CASES.index(case))
    if kind == "stem":
        views = 1 if which == "one" else many_views(cu)
        if which == "many":
            tiles = views * STEM_TILES
            assert tiles > 4 * cu and all(tiles % (k * cu) for k in (2, 3, 4)), (tiles, cu)
        images = torch.rand((views, STEM_H, STEM_W, 3), generator=g) * 2.0 - 0.75
        return sha(eng.forward_upto(images.to(device), 1))
    frames = torch.randint(0, 256, U8_FRAMES[which], dtype=torch.uint8, generator=g).to(device)
    flip = torch.tensor(U8_FLIP, dtype=torch.uint8, device=device)
    return sha(eng.forward_u8(frames, flip, U8_MEAN, U8_STD))


@pytest.fixture(scope="module")
def engines():
    return {}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    omitted = fx["omitted"]
    # a case that did not repeat at the commit the digests were recorded at may be left out: none of the stem outputs, one forward_u8 case
    assert not [n for n in omitted if n.startswith("stem")] and len(omitted) <= 1, omitted
    assert sorted(list(fx["digests"]) + omitted) == sorted(case_name(c) for c in CASES)
    return fx


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_stem_output_is_unchanged(cuda, engines, recorded, case):
    import torch

    name = case_name(case)
    if name in recorded["omitted"]:
        pytest.skip(f"{name}: not reproducible where the digests were recorded")
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    if case[2] == "many" and cu != recorded["cu"]:
        pytest.skip(f"{name}: the view count follows from the CU count; recorded on {recorded['cu']} CUs, this device has {cu}")
    got = digest(case, engines, cuda, cu)
    assert got == recorded["digests"][name], f"{name}: the output changed"


if __name__ == "__main__":
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    engines = {}
    fx = {"cu": cu, "omitted": [], "digests": {case_name(c): digest(c, engines, torch.device("cuda:0"), cu) for c in CASES}}
    with open(out, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print(json.dumps(fx, indent=1))
