"""-m gpu: the camera front-end -- df3d_preprocess_u8 (csrc/preprocess.hip) and the stems' own sampling of uint8 frames (df3d_pre::pixel
called from csrc/hg_stem.h behind df3d_hg_forward_u8) -- swept over frame and output shapes.

tests/test_gpu_core.py covers the product's case: one network input size (256 x 512), down-scales only, the three resize rules on the
f32 engine and the four dtypes on `bilinear`.  The per-pixel arithmetic (csrc/preprocess_math.h) is sound on up-scales, 1 x 1 frames,
1 x 1 outputs and identity sizes too; what this file is after is the code AROUND the sampler: the index decomposition and the view
offset of preprocess_kernel, the flip table, the tail of the last block, and the u8 gather of the three stem kernels on tile grids other
than 32 x 16, on the single-tile path and on the next-tile-prefetch path of stem_walk.

The oracle is oracle/preprocess.py, and it has to stay that: the rule's source coordinates are float32 BY DEFINITION (torch's
interpolate computes them in float32, and so does the kernel).  A "more exact" bilinear with float64 coordinates is a different
function: on noise images it differs from the rule by up to 3.8e-5 for that reason alone, nineteen times the bound used here.  Do
not upgrade the oracle to one.

Bound: 2e-6 absolute, the project's own (test_every_resize_rule_against_its_restatement): the values are O(1) and about ten float32
roundings deep; the same arithmetic compiled for the host stays at or below 7.2e-7 on these shapes with mean 0 and std 1, and the
kernel at or below 8.4e-7 with the mean and std used here (each case prints its figure).  Where no oracle is needed -- at the identity
size and on a 1 x 1 frame every rule returns the normalised source pixel -- the comparison is bit for bit; that holds only while
multiply-add fusion is really off in df3d_pre::pixel (csrc/preprocess_math.h and the file flags of deepfly3d_amd/build.py)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import preprocess as opre

pytestmark = pytest.mark.gpu

MEAN, STD = (0.22, 0.31, 0.18), (0.9, 1.1, 1.3)   # as in tests/test_gpu_core.py
TOL = 2e-6
N_VIEWS, FLIP7 = 7, [0, 1, 1, 0, 1, 0, 0]
SHAPES = [((1, 1), (8, 8)), ((1, 7), (4, 4)), ((5, 1), (4, 4)), ((30, 50), (64, 128)), ((64, 128), (64, 128)), ((100, 30), (30, 9)), ((33, 17), (1, 1)),
          ((7, 250), (64, 64)), ((2, 2), (64, 64)), ((300, 400), (200, 256)), ((63, 65), (64, 64)), ((1000, 30), (3, 64))]
RAGGED = [s for s in SHAPES if (N_VIEWS * s[1][0] * s[1][1]) % 256]   # the last block of the launch has idle threads
assert len(RAGGED) >= 3
GUARD, POISON = 4096, 0xA5
EINVAL = -1   # DF3D_EINVAL of include/df3d_hip.h


class rule_set:
    """inference.PREPROCESS for the duration of a block, restored whatever happens."""

    def __init__(self, rule):
        self.rule = rule

    def __enter__(self):
        from deepfly3d_amd import inference

        self.saved = dict(inference.PREPROCESS)
        inference.PREPROCESS.update(mean=MEAN, std=STD, resize=self.rule)

    def __exit__(self, *exc):
        from deepfly3d_amd import inference

        inference.PREPROCESS.clear()
        inference.PREPROCESS.update(self.saved)


def _frames(seed, n, hw, C):
    """[n, H, W] (C = 1) or [n, H, W, 3] uint8 noise: every view and every channel has content of its own."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, *hw) if C == 1 else (n, *hw, C), dtype=torch.uint8, generator=g)


def _normalised(v_u8, flip):
    """[n, H, W, C] uint8 -> what every rule returns at the identity size, in numpy float32 with the kernel's operations:
    ((v * (1 / 255)) - mean) * (1 / std), the two reciprocals taken in float32."""
    v = v_u8.numpy()
    if v.ndim == 3:
        v = v[..., None]
    v = np.where(np.asarray(flip, bool)[:, None, None, None], v[:, :, ::-1], v)
    v = np.broadcast_to(v, (*v.shape[:3], 3)).astype(np.float32)
    one = np.float32(1.0)
    return (v * (one / np.float32(255.0)) - np.asarray(MEAN, np.float32)) * (one / np.asarray(STD, np.float32))


# ---- df3d_preprocess_u8 against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", opre.RESIZE_RULES)
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_preprocess_over_shapes_rules_channels_and_flips(native_lib, cuda, src, dst, rule):
    from deepfly3d_amd import inference

    flip = torch.tensor(FLIP7, dtype=torch.uint8)
    with rule_set(rule):
        for C in (1, 3):
            frames = _frames(100 * src[0] + src[1] + C, N_VIEWS, src, C)
            got = inference.preprocess_u8(frames.to(cuda), flip.to(cuda), dst).cpu()
            ref = opre.preprocess_u8(frames, flip, dst, MEAN, STD, rule)
            assert got.shape == (N_VIEWS, *dst, 3) and got.dtype == torch.float32
            err = float((got - ref).abs().max())
            print(f"{rule} C={C} {src} -> {dst}: max abs err {err:.3g}")
            assert err < TOL, (rule, C, src, dst, err)
            if src[1] > 1:
                assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])   # the views differ: an offset slip would show
            # no flip table = a table of zeros
            none = inference.preprocess_u8(frames.to(cuda), None, dst)
            assert torch.equal(none, inference.preprocess_u8(frames.to(cuda), torch.zeros(N_VIEWS, dtype=torch.uint8, device=cuda), dst))
            assert float((none.cpu() - opre.preprocess_u8(frames, None, dst, MEAN, STD, rule)).abs().max()) < TOL
            if C == 3:
                assert not torch.equal(got[..., 0] * STD[0] + MEAN[0], got[..., 1] * STD[1] + MEAN[1])   # the channels are read, each its own


@pytest.mark.parametrize("rule", opre.RESIZE_RULES)
def test_the_identity_size_returns_the_normalised_pixels_bit_for_bit(native_lib, cuda, rule):
    from deepfly3d_amd import inference

    assert np.float32(1.0) / np.float32(255.0) == np.float32(1 / 255)
    with rule_set(rule):
        for hw in ((64, 128), (5, 7), (1, 300)):
            for C in (1, 3):
                frames = _frames(hw[1] + C, N_VIEWS, hw, C)
                for flip in (FLIP7, [0] * N_VIEWS):
                    got = inference.preprocess_u8(frames.to(cuda), torch.tensor(flip, dtype=torch.uint8, device=cuda), hw).cpu().numpy()
                    assert np.array_equal(got, _normalised(frames, flip)), (rule, hw, C, flip)


@pytest.mark.parametrize("rule", opre.RESIZE_RULES)
def test_a_one_pixel_frame_gives_a_constant_image(native_lib, cuda, rule):
    """(`area` on output sizes that are powers of two only: its overlap weights 1 / OH and 1 / OW are then exact, and so is their product
    with the reciprocal of the covered area; at 3 x 70 that product is 1 up to rounding, which is the oracle comparison's business.)"""
    from deepfly3d_amd import inference

    with rule_set(rule):
        for C in (1, 3):
            frames = _frames(40 + C, N_VIEWS, (1, 1), C)
            for dst in ((8, 8), (1, 1), (4, 64)) + (((3, 70),) if rule != "area" else ()):
                got = inference.preprocess_u8(frames.to(cuda), torch.tensor(FLIP7, dtype=torch.uint8, device=cuda), dst).cpu().numpy()
                want = np.broadcast_to(_normalised(frames, FLIP7), (N_VIEWS, *dst, 3))
                assert np.array_equal(got, want), (rule, C, dst)


# ---- through the C ABI: guard words, n = 0, refusals, a side stream ------------------------------------------------------------------------
def _call(lib, cuda, frames_d, flip_d, n, H, W, C, out_p, OH, OW, resize, mean=MEAN, std=STD, stream=None):
    with torch.cuda.device(cuda):
        return lib.df3d_preprocess_u8(frames_d.data_ptr() if frames_d is not None else None, flip_d.data_ptr() if flip_d is not None else None, n, H, W, C,
                                      out_p, OH, OW, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), resize,
                                      torch.cuda.current_stream(cuda).cuda_stream if stream is None else stream)


def _guarded(cuda, nbytes):
    buf = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=cuda)
    return buf, buf.data_ptr() + GUARD


@pytest.mark.parametrize("rule", opre.RESIZE_RULES)
@pytest.mark.parametrize("src,dst", RAGGED + [((64, 128), (64, 128))], ids=lambda v: f"{v[0]}x{v[1]}")
def test_every_float_of_the_output_is_written_and_nothing_else(native_lib, cuda, src, dst, rule):
    from deepfly3d_amd import _native, inference

    for C in (1, 3):
        frames = _frames(7 + C, N_VIEWS, src, C).to(cuda)
        flip = torch.tensor(FLIP7, dtype=torch.uint8, device=cuda)
        nfloat = N_VIEWS * dst[0] * dst[1] * 3
        buf, out_p = _guarded(cuda, 4 * nfloat)
        assert out_p % 16 == 0
        assert _call(native_lib, cuda, frames, flip, N_VIEWS, *src, C, out_p, *dst, _native.RESIZE_MODES[rule]) == 0, native_lib.df3d_last_error()
        host = buf.cpu().numpy()
        assert (host[:GUARD] == POISON).all() and (host[GUARD + 4 * nfloat:] == POISON).all(), "bytes outside the output were written"
        words = host[GUARD:GUARD + 4 * nfloat].view(np.uint32)
        assert (words != 0xA5A5A5A5).all(), "a float of the output was not written"
        with rule_set(rule):
            want = inference.preprocess_u8(frames, flip, dst).cpu().numpy()
        assert np.array_equal(words.view(np.float32).reshape(want.shape), want)


def test_no_views_no_launch_and_the_refusals(native_lib, cuda):
    frames = _frames(3, 2, (5, 6), 3).to(cuda)
    two = torch.zeros((2, 5, 6, 2), dtype=torch.uint8, device=cuda)
    buf, out_p = _guarded(cuda, 4 * 2 * 4 * 4 * 3)

    def untouched():
        torch.cuda.synchronize(cuda)
        return bool((buf.cpu().numpy() == POISON).all())

    assert _call(native_lib, cuda, frames, None, 0, 5, 6, 3, out_p, 4, 4, 0) == 0 and untouched()
    assert _call(native_lib, cuda, None, None, 0, 5, 6, 3, None, 4, 4, 0) == 0   # with no views the pointers are not looked at
    for what, rc in {
        "C = 2": _call(native_lib, cuda, two, None, 2, 5, 6, 2, out_p, 4, 4, 0),
        "std = 0": _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 4, 4, 0, std=(0.9, 0.0, 1.3)),
        "resize = 3": _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 4, 4, 3),
        "resize = -1": _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 4, 4, -1),
        "n = -1": _call(native_lib, cuda, frames, None, -1, 5, 6, 3, out_p, 4, 4, 0),
        "OH = 0": _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 0, 4, 0),
        "no frames": _call(native_lib, cuda, None, None, 2, 5, 6, 3, out_p, 4, 4, 0),
        "no output": _call(native_lib, cuda, frames, None, 2, 5, 6, 3, None, 4, 4, 0),
    }.items():
        assert rc == EINVAL, (what, rc)
    # (each refusal left a message; the last one's is still there)
    assert _call(native_lib, cuda, frames, None, 2, 5, 6, 2, out_p, 4, 4, 0) == EINVAL and b"C must be 1 or 3" in native_lib.df3d_last_error()
    assert _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 4, 4, 0, std=(0.0, 1.0, 1.0)) == EINVAL and b"std" in native_lib.df3d_last_error()
    assert _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 4, 4, 3) == EINVAL and b"resize" in native_lib.df3d_last_error()
    assert untouched()
    assert _call(native_lib, cuda, frames, None, 2, 5, 6, 3, out_p, 4, 4, 0) == 0 and not untouched()   # the valid call these were derived from


def test_a_side_stream_run_repeats_bit_for_bit(native_lib, cuda):
    from deepfly3d_amd import inference

    frames, flip = _frames(9, N_VIEWS, (100, 30), 3).to(cuda), torch.tensor(FLIP7, dtype=torch.uint8, device=cuda)
    with rule_set("area"):
        want = inference.preprocess_u8(frames, flip, (30, 9))
        torch.cuda.synchronize(cuda)
        side = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(cuda).cuda_stream == side.cuda_stream and side.cuda_stream != 0
            a = inference.preprocess_u8(frames, flip, (30, 9))
            b = inference.preprocess_u8(frames, flip, (30, 9))
        side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, want)


# ---- the u8 stems: forward_u8(frames) == forward(preprocess_u8(frames)), bit for bit ---------------------------------------------------------
ENGINE_SIZES = [(64, 64), (128, 64), (64, 192)]   # 4 x 2, 8 x 2 and 4 x 6 stem tiles per view (a tile is 8 x 16 output pixels = 16 x 32 input pixels)
DTYPES = ["f32", "f32s", "bf16", "f16"]
STEM_TILES_64 = (64 // 2 // 8) * (64 // 2 // 16)   # 8 per view


@pytest.fixture(scope="module")
def weights():
    from deepfly3d_amd.synthetic import synthetic_state_dict

    return synthetic_state_dict(3)


@pytest.fixture(scope="module")
def engines(cuda, weights):
    """(dtype, height, width) -> HourglassEngine, built at first use and kept for the module"""
    from deepfly3d_amd.hourglass import HourglassEngine

    made = {}

    def get(dtype, height, width):
        if (dtype, height, width) not in made:
            made[(dtype, height, width)] = HourglassEngine(weights, dtype=dtype, device=cuda, height=height, width=width)
        return made[(dtype, height, width)]

    return get


def _stem_frames(n, hw):
    """name -> [n, ...] uint8 frames: an up-scale from grey, the engine's own size in colour (the identity), a colour frame of odd size, one pixel"""
    return {"30x50 grey": _frames(1, n, (30, 50), 1), "own size": _frames(2, n, hw, 3), "101x77 colour": _frames(3, n, (101, 77), 3), "1x1": _frames(4, n, (1, 1), 1)}


def _check_stem(eng, cuda, n, hw):
    from deepfly3d_amd import inference

    flip = torch.tensor(([1, 0, 0, 1, 1] * (n // 5 + 1))[:n], dtype=torch.uint8, device=cuda)
    for rule in opre.RESIZE_RULES:
        with rule_set(rule):
            for name, frames in _stem_frames(n, hw).items():
                frames = frames.to(cuda)
                outs = {}
                for fl in (flip, None):
                    ref = eng.forward(inference.preprocess_u8(frames, fl, hw))
                    got = eng.forward_u8(frames, fl, MEAN, STD, resize=rule)
                    assert got.shape == (n, 19, hw[0] // 4, hw[1] // 4)
                    assert torch.equal(ref, got), (eng.dtype, hw, n, rule, name, "flip" if fl is not None else "no flip")
                    outs[fl is None] = got
                if name != "1x1":
                    assert not torch.equal(outs[False], outs[True])   # the flip table is read: view 0 is mirrored


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", ENGINE_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_u8_stem_equals_preprocess_then_forward_on_one_view(native_lib, cuda, engines, hw, dtype):
    """n = 1: at most 48 tiles, fewer than any stem grid has workgroups, so every workgroup has one tile and none prefetches."""
    _check_stem(engines(dtype, *hw), cuda, 1, hw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_u8_stem_equals_preprocess_then_forward_where_workgroups_walk_on(native_lib, cuda, engines, dtype):
    """The stems are persistent: launch_stem_step (csrc/hg_launch.h) starts min(tiles, k * CUs) workgroups, k = 3 (f32), 4 (bf16, f16) or 2
    (f32s) per CU, and workgroup b walks tiles b, b + grid, ...; a tile after a workgroup's first is gathered -- with the u8 sampling --
    BEHIND the previous tile's K loop and scattered between two barriers (stem_walk, csrc/hg_stem.h).  At 64 x 64 a view has 8 tiles, so
    n = 4 CUs // 8 + 3 views (131 on 256 CUs: 1048 tiles) is more tiles than the largest of the three grids (1024) and no whole number
    of rounds of any of them: every stem prefetches, and ends on a partial round."""
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = 4 * cu // STEM_TILES_64 + 3
    tiles = n * STEM_TILES_64
    assert tiles > 4 * cu and all(tiles % (k * cu) for k in (2, 3, 4)), (tiles, cu)
    _check_stem(engines(dtype, 64, 64), cuda, n, (64, 64))
