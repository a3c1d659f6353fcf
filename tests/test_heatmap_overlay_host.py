"""CPU tests of the heat-map overlays: properties of the float64 oracle that fixes the drawing rule, the
camera -> plane -> joint table, the CLI flag and the argument validation of the new C entry (no device is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

import heatmap_overlay_oracle as ho

H, W, HH, WH = 480, 960, 64, 128


def _peak_plane(r, c):
    hm = np.zeros((1, HH, WH), np.float32)
    hm[0, r, c] = 1.0
    return hm


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("r,c", [(0, 0), (1, 1), (10, 21), (11, 20), (33, 64), (62, 126), (61, 125)])
def test_single_peak_lands_where_the_detection_is_drawn(r, c, flip):
    """A plane that is 1 at one cell: the pixel of largest alpha lies within 1 px of the pixel plot_2d draws that arg-max at,
    (r H / Hh, c W / Wh) = (7.5 r, 7.5 c), and for a mirrored view at column W - 7.5 c (the re-layout's col -> 1 - col).  c = 0
    flipped is column W, outside the image: its nearest pixel is W - 1, which reads the clamped last column."""
    a = ho.alpha(_peak_plane(r, c), [0], H, W, flip)[0]
    y, x = np.unravel_index(int(a.argmax()), a.shape)
    want_y, want_x = r * 7.5, (W - c * 7.5) if flip else c * 7.5
    print(f"peak ({r}, {c}) flip {flip}: alpha max {a.max():.4f} at ({y}, {x}), detection drawn at ({want_y}, {want_x})")
    assert a.max() > 0.8
    assert abs(y - want_y) <= 1.0 and abs(x - want_x) <= 1.0
    # every pixel that reaches the maximum is that near (the maximum is not a plateau somewhere else)
    ys, xs = np.nonzero(a == a.max())
    assert np.all(np.abs(ys - want_y) <= 1.0) and np.all(np.abs(xs - want_x) <= 1.0)


@pytest.mark.parametrize("flip", [False, True])
def test_last_row_and_column_extend_to_the_image_edge(flip):
    """Past the last cell the taps are clamped (i1 = min(i0 + 1, n - 1)), so a peak in the last row / column keeps its value from the
    pixel of the detection to the edge of the image: the pixels beside the detection are among the maxima, and nothing further inside is."""
    a = ho.alpha(_peak_plane(63, 127), [0], H, W, flip)[0]
    ys, xs = np.nonzero(a == a.max())
    want_x = (W - 127 * 7.5) if flip else 127 * 7.5
    assert ys.min() == 473 and ys.max() == H - 1          # 63 * 7.5 = 472.5
    assert (xs.min(), xs.max()) == ((0, 7) if flip else (953, W - 1))
    assert np.abs(ys - 472.5).min() <= 1.0 and np.abs(xs - want_x).min() <= 1.0


def test_flipped_column_w_reads_the_clamped_last_column():
    hm = np.zeros((1, 4, 8), np.float32)
    hm[0, :, 7] = 0.5
    a = ho.alpha(hm, [0], 30, 52, True)[0]
    # x = 0 flipped is xs = W: sx = Wh, past the last cell, so the tap is the last column alone
    assert np.all(a[:, 0] == 0.5)
    assert np.all(ho.alpha(hm, [0], 30, 52, False)[0][:, 0] == 0.0)


def test_nothing_selected_or_all_nan_is_the_grey_image():
    rng = np.random.default_rng(0)
    luma = rng.integers(0, 256, size=(30, 52), dtype=np.uint8)
    grey = np.repeat(luma[:, :, None], 3, axis=2)
    hm = rng.random((3, 4, 8), dtype=np.float32)
    assert np.array_equal(ho.overlay_view(luma, hm, [], [], False), grey)
    hm[1] = np.nan
    assert np.array_equal(ho.overlay_view(luma, hm, [1], [(255, 0, 0)], True), grey)
    assert not np.array_equal(ho.overlay_view(luma, hm, [0], [(255, 0, 0)], True), grey)
    # gain 0 and non-positive planes contribute nothing either
    assert np.array_equal(ho.overlay_view(luma, hm, [0, 2], [(255, 0, 0), (0, 255, 0)], False, gain=0.0), grey)
    assert np.array_equal(ho.overlay_view(luma, -hm, [0, 2], [(255, 0, 0), (0, 255, 0)], False), grey)


def test_ties_go_to_the_earliest_selected_plane_and_alpha_blends():
    luma = np.full((8, 8), 100, np.uint8)
    hm = np.full((2, 2, 2), 0.5, np.float32)
    out = ho.overlay_view(luma, hm, [1, 0], [(200, 0, 50), (0, 200, 0)], False)
    assert np.all(out == np.array([150, 50, 75], np.uint8))       # floor(0.5 * 100 + 0.5 * C + 0.5), the first listed plane's colour
    out = ho.overlay_view(luma, hm, [1, 0], [(200, 0, 50), (0, 200, 0)], False, gain=4.0)
    assert np.all(out == np.array([200, 0, 50], np.uint8))        # clamped to 1: the colour itself


def test_heatmap_planes_follow_the_relayout():
    from deepfly3d_amd.config import LIMB_COLORS, heatmap_planes, limb_of_joint, plane_color

    for pos in (0, 1):
        assert heatmap_planes(pos) == [(p, p) for p in range(19)]
    assert heatmap_planes(2) == [(p, p) for p in range(15)]
    assert heatmap_planes(3) == []
    assert heatmap_planes(4) == [(p, p + 19) for p in range(15)]
    for pos in (5, 6):
        assert heatmap_planes(pos) == [(p, p + 19) for p in range(19)]
    # `joints` filters by 38-layout id and keeps plane order, whatever the order of the list
    assert heatmap_planes(0, joints=[18, 4, 7]) == [(4, 4), (7, 7), (18, 18)]
    assert heatmap_planes(5, joints=[37, 19]) == [(0, 19), (18, 37)]
    # joints the camera does not fill are dropped: the other side's, the stripes of positions 2 and 4, everything for the front camera
    assert heatmap_planes(0, joints=[20, 3]) == [(3, 3)]
    assert heatmap_planes(2, joints=[16, 14]) == [(14, 14)]
    assert heatmap_planes(4, joints=[34, 33]) == [(14, 33)]
    assert heatmap_planes(3, joints=[5, 24]) == []
    assert heatmap_planes(6, joints=[5]) == []
    # the table is keyed on the camera's position in the ordering
    order = [6, 5, 4, 3, 2, 1, 0]
    assert heatmap_planes(6, camera_ordering=order) == [(p, p) for p in range(19)]
    assert heatmap_planes(4, camera_ordering=order) == [(p, p) for p in range(15)]
    assert heatmap_planes(2, camera_ordering=order) == [(p, p + 19) for p in range(15)]
    assert heatmap_planes(3, camera_ordering=order) == []
    with pytest.raises(NotImplementedError):
        heatmap_planes(7)
    for j in (0, 7, 15, 18, 19, 30, 37):
        assert tuple(plane_color(j)) == tuple(LIMB_COLORS[limb_of_joint(j)])


def test_heatmap_planes_agree_with_the_relayout_oracle():
    """The pairs are exactly the (source plane, joint) the re-layout fills, for the identity and a reversed ordering."""
    from oracle import geometry as og

    from deepfly3d_amd.config import camera_is_flipped, heatmap_planes

    pts = np.zeros((7, 1, 19, 2), np.float32)
    pts[..., 0] = (np.arange(19, dtype=np.float32) + 1) / 64     # row tags the plane
    pts[..., 1] = 0.25
    for order in ([0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0], [0, 6, 5, 4, 3, 2, 1]):
        out = og.relayout_19_to_38(pts, order)
        for cam in range(7):
            filled = [(int(round(out[cam, 0, j, 0] * 64)) - 1, j) for j in range(38) if out[cam, 0, j, 0] != 0]
            assert heatmap_planes(cam, camera_ordering=order) == filled
            if filled:
                assert camera_is_flipped(cam, order) == (out[cam, 0, filled[0][1], 1] == 0.75)


def test_cli_video_heatmap_flag():
    from deepfly3d_amd.cli import parse_cli_args

    assert parse_cli_args(["/tmp/x", "--video-heatmap"]).video_heatmap is True
    assert parse_cli_args(["/tmp/x"]).video_heatmap is False
    a = parse_cli_args(["/tmp/x", "--video-heatmap", "--skip-pose-estimation"])
    assert a.video_heatmap is True and a.skip_estimation is True
    a = parse_cli_args(["/tmp/x", "--video-heatmap", "--video-2d", "--video-3d"])
    assert a.video_heatmap and a.video_2d and a.video_3d


def test_cli_refuses_the_heatmap_video_without_images(tmp_path):
    """After --delete-images there are no frames to compute heat-maps from, and heat-maps are never stored: the run says so before it
    touches the device."""
    from deepfly3d_amd import cli

    folder = tmp_path / "images"
    folder.mkdir()
    args = cli.parse_cli_args([str(folder), "--video-heatmap", "--skip-pose-estimation", "--output-folder", str(tmp_path / "out")])
    with pytest.raises(FileNotFoundError, match="--delete-images.*never stored"):
        cli.run(args)
    assert not (tmp_path / "out").exists()


def test_header_and_prototypes_declare_the_entry(native_lib):
    from deepfly3d_amd import _native

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "df3d_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+df3d_render_heatmap\s*\(", text)
    assert "df3d_render_heatmap" in _native.PROTOTYPES and hasattr(native_lib, "df3d_render_heatmap")
    assert len(_native.PROTOTYPES["df3d_render_heatmap"][1]) == 16
    assert native_lib.df3d_version() == 610   # additive: the revision stays


def test_entry_validates_arguments_without_gpu(native_lib):
    lib = native_lib
    fn = lib.df3d_render_heatmap
    p = ctypes.c_void_p(4096)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)       # noqa: E731
    bytes_ = lambda *v: (ctypes.c_ubyte * len(v))(*v)   # noqa: E731
    one, plane0, red, noflip = ints(1), ints(0), bytes_(255, 0, 0), bytes_(0)

    def call(luma=p, h=30, w=52, hm=p, planes=19, hh=4, wh=8, slots=1, cols=1, n=one, sel=plane0, rgb=red, flip=noflip, gain=1.0, out=p):
        return fn(luma, h, w, hm, planes, hh, wh, slots, cols, n, sel, rgb, flip, gain, out, None)

    for bad in (dict(slots=0), dict(slots=9, cols=3), dict(cols=0), dict(cols=2)):
        assert call(**bad) == -1 and b"slots" in lib.df3d_last_error()
    for bad in (dict(h=0), dict(w=-1), dict(planes=0), dict(hh=0), dict(wh=0)):
        assert call(**bad) == -1 and b"positive" in lib.df3d_last_error()
    assert call(h=65536) == -1 and b"too large" in lib.df3d_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert call(gain=bad) == -1 and b"gain" in lib.df3d_last_error()
    for bad in (dict(luma=None), dict(hm=None), dict(out=None), dict(n=None), dict(flip=None), dict(sel=None), dict(rgb=None)):
        assert call(**bad) == -1 and b"null" in lib.df3d_last_error()
    assert call(n=ints(33)) == -1 and b"0..32" in lib.df3d_last_error()
    assert call(n=ints(-1)) == -1 and b"0..32" in lib.df3d_last_error()
    assert call(sel=ints(19)) == -1 and b"plane index" in lib.df3d_last_error()
    assert call(sel=ints(-1)) == -1 and b"plane index" in lib.df3d_last_error()
    # the second slot's tables are read behind the first slot's
    assert call(slots=2, cols=2, n=ints(1, 1), sel=ints(0, 19), rgb=bytes_(1, 2, 3, 4, 5, 6), flip=bytes_(0, 1)) == -1 and b"plane index" in lib.df3d_last_error()


def test_python_entry_refuses_cpu_tensors_and_bad_tables():
    torch = pytest.importorskip("torch")
    from deepfly3d_amd import ops

    luma, hm = torch.zeros((1, 30, 52), dtype=torch.uint8), torch.zeros((1, 19, 4, 8))
    with pytest.raises(ValueError):
        ops.render_heatmap(luma, hm, [[0]], [[(255, 0, 0)]], [False])   # the kernel runs on the device only
