"""-m gpu: the heat-map overlays -- df3d_render_heatmap against the float64 oracle bit for bit, Core.heatmaps /
Core.plot_heatmap against the run's own detections, and `df3d-cli --video-heatmap` end to end on the golden frames."""
import os
import shutil

import numpy as np
import pytest
import torch

import heatmap_overlay_oracle as ho

pytestmark = pytest.mark.gpu

PALETTE = [(186, 30, 49), (15, 115, 153), (210, 210, 210), (0, 255, 0), (255, 255, 255), (0, 0, 0), (213, 133, 121), (117, 190, 203)]


def _colors(n, shift=0):
    return [PALETTE[(k + shift) % len(PALETTE)] for k in range(n)]


def _render(cuda, luma, hm, sels, colors, flips, **kw):
    from deepfly3d_amd import ops

    return ops.render_heatmap(torch.from_numpy(luma).to(cuda), torch.from_numpy(hm).to(cuda), sels, colors, flips, **kw)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("sel", [[3], [4, 0, 2]])
def test_ragged_view_equals_the_oracle(native_lib, cuda, sel, flip):
    """30 x 52 over 4 x 8 maps: a non-integer ratio (7.5 and 6.5 px per cell), a width below one 256-thread block."""
    rng = np.random.default_rng(10)
    luma = rng.integers(0, 256, size=(1, 30, 52), dtype=np.uint8)
    hm = rng.uniform(-0.2, 1.2, size=(1, 5, 4, 8)).astype(np.float32)
    got = _render(cuda, luma, hm, [sel], [_colors(len(sel))], [flip]).cpu().numpy()
    ref = ho.overlay_view(luma[0], hm[0], sel, _colors(len(sel)), flip)
    assert got.shape == (30, 52, 3) and got.dtype == np.uint8 and np.array_equal(got, ref)
    assert (got != luma[0][:, :, None]).any()   # something was drawn
    # the single-view form of the call
    from deepfly3d_amd import ops

    one = ops.render_heatmap(torch.from_numpy(luma[0]).to(cuda), torch.from_numpy(hm[0]).to(cuda), sel, _colors(len(sel)), flip).cpu().numpy()
    assert np.array_equal(one, ref)


def test_video_grid_equals_the_oracle(native_lib, cuda):
    """The video frame's shape: six 480 x 960 views over 64 x 128 maps in three columns, the bottom row mirrored, all 19 planes on some
    views and none on another."""
    rng = np.random.default_rng(11)
    luma = rng.integers(0, 256, size=(6, 480, 960), dtype=np.uint8)
    hm = rng.uniform(-0.3, 1.1, size=(6, 19, 64, 128)).astype(np.float32)
    sels = [list(range(19)), [], [18, 3, 7], list(range(18, -1, -1)), [5, 5], [0, 2, 4, 6, 8]]
    colors = [_colors(len(s), k) for k, s in enumerate(sels)]
    flips = [0, 0, 0, 1, 1, 1]
    got = _render(cuda, luma, hm, sels, colors, flips, cols=3).cpu().numpy()
    ref = ho.overlay_grid(luma, hm, sels, colors, flips, cols=3)
    assert got.shape == (960, 2880, 3) and np.array_equal(got, ref)
    assert np.array_equal(got[:480, 960:1920], np.repeat(luma[1][:, :, None], 3, axis=2))   # nothing selected: the grey image


@pytest.mark.parametrize("gain", [1.0, 2.5])
def test_edge_values_equal_the_oracle(native_lib, cuda, gain):
    """17 x 300 (a width that is no multiple of the 256-thread block) over 5 x 7 maps holding values below 0 and above 1, NaN, +inf, -inf
    and two selected planes that are equal everywhere (an exact tie at every pixel: the earlier one's colour)."""
    rng = np.random.default_rng(12)
    luma = rng.integers(0, 256, size=(2, 17, 300), dtype=np.uint8)
    hm = rng.uniform(-0.5, 1.5, size=(2, 6, 5, 7)).astype(np.float32)
    hm[:, 1, 2, 3] = np.nan
    hm[:, 1, 0, 0] = np.inf
    hm[:, 3, 4, 6] = np.inf
    hm[:, 3, 1, 1] = -np.inf
    hm[:, 3, 2, 5] = 3.0e38
    hm[:, 4] = hm[:, 0]                              # ties with plane 0 everywhere
    hm[:, 5] = np.where(hm[:, 2] > 0.5, hm[:, 2], 0.25)   # ties with plane 2 on part of the image
    sels = [[4, 0, 1, 3], [2, 5, 0, 4, 3, 1]]
    colors = [_colors(4), _colors(6, 3)]
    flips = [False, True]
    got = _render(cuda, luma, hm, sels, colors, flips, gain=gain, cols=1).cpu().numpy()
    ref = ho.overlay_grid(luma, hm, sels, colors, flips, gain=gain, cols=1)
    assert got.shape == (34, 300, 3) and np.array_equal(got, ref)
    # the tie went to the earlier plane everywhere: the frame is the one drawn without plane 0, which is listed after its equal
    only0 = ho.overlay_view(luma[0], hm[0], [4, 1, 3], [colors[0][0]] + colors[0][2:], False, gain)
    assert np.array_equal(got[:17], only0)


def test_bytes_past_the_frame_stay_untouched(native_lib, cuda):
    rng = np.random.default_rng(13)
    luma = rng.integers(0, 256, size=(5, 30, 52), dtype=np.uint8)
    hm = rng.uniform(-0.2, 1.2, size=(5, 5, 4, 8)).astype(np.float32)
    sels = [[0], [1, 2], [], [4, 3], [2]]
    colors = [_colors(len(s), k) for k, s in enumerate(sels)]
    flips = [0, 1, 0, 1, 1]
    need = 2 * 30 * 3 * 52 * 3
    out = torch.full((need + 4096,), 0xAB, dtype=torch.uint8, device=cuda)
    frame = _render(cuda, luma, hm, sels, colors, flips, cols=3, out=out)
    assert frame.shape == (60, 156, 3) and frame.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    assert np.all(host[need:] == 0xAB)
    # five views in a 2 x 3 grid: the sixth cell is not written either
    assert np.array_equal(host[:need].reshape(60, 156, 3), ho.overlay_grid(luma, hm, sels, colors, flips, cols=3, fill=0xAB))
    # a tensor made by the call has that cell zeroed
    assert np.array_equal(_render(cuda, luma, hm, sels, colors, flips, cols=3).cpu().numpy(), ho.overlay_grid(luma, hm, sels, colors, flips, cols=3, fill=0))
    with pytest.raises(ValueError):
        _render(cuda, luma, hm, sels, colors, flips, cols=3, out=out[: need - 1])


# ---- Core and the CLI on the two golden frames, synthetic weights -------------------------------------------------------------------
def _copy_images(golden_dir, folder):
    os.makedirs(folder)
    for f in os.listdir(os.path.join(golden_dir, "images")):
        shutil.copy(os.path.join(golden_dir, "images", f), folder)
    return folder


def _result_bytes(folder):
    out_dir = folder + "_df3d"
    names = [f for f in os.listdir(out_dir) if f.startswith("df3d_result")]
    assert len(names) == 1
    with open(os.path.join(out_dir, names[0]), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def plain_run(native_lib, cuda, tmp_path_factory, golden_dir):
    """One `df3d-cli INPUT -n 2` run without the new flag (its result pickle is the baseline), then a Core on the same folder with a
    plain f32 pose2d_estimation()."""
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
        config.pop("image_shape", None)
        folder = _copy_images(golden_dir, str(tmp_path_factory.mktemp("plain") / "images"))
        assert cli.main([folder, "-n", "2"]) == 0
        baseline = _result_bytes(folder)
        core = Core(folder, None, 2)
        core.pose2d_estimation()
        yield core, folder, baseline
        config.pop("image_shape", None)


def test_core_heatmaps_are_the_ones_the_run_used(plain_run, cuda):
    """Every detection of the run is the arg-max of its plane of Core.heatmaps(), un-flipped as the re-layout does it: this pins the
    camera -> plane -> joint table and the flip set, and shows that the heat-maps are recomputed exactly."""
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import camera_is_flipped, heatmap_planes

    core, _, _ = plain_run
    checked = 0
    for t in range(2):
        hm = core.heatmaps(t)
        assert hm.is_cuda and hm.dtype == torch.float32 and tuple(hm.shape) == (7, 19, 64, 128)
        assert core.heatmaps(t) is hm   # the one-entry cache
        pts = ops.heatmap_argmax(hm)[0].cpu().numpy()   # [7, 19, 2] float32 (row / 64, col / 128)
        for c in range(7):
            pairs = heatmap_planes(c, camera_ordering=core.camera_ordering)
            filled = {j for _, j in pairs}
            for plane, j in pairs:
                row, col = np.float64(pts[c, plane, 0]), np.float64(pts[c, plane, 1])
                if camera_is_flipped(c, core.camera_ordering):
                    col = 1.0 - col
                assert core.points2d[c, t, j, 0] == row and core.points2d[c, t, j, 1] == col, (c, t, j)
                checked += 1
            for j in range(38):
                if j not in filled:
                    assert core.points2d[c, t, j, 0] == 0.0   # no plane fills it
    assert checked == 2 * (4 * 19 + 2 * 15)
    assert np.any(core.points2d[:, :2] != 0)


def test_plot_heatmap_equals_the_oracle(plain_run, cuda):
    from deepfly3d_amd import jpeg
    from deepfly3d_amd.config import camera_is_flipped, heatmap_planes, plane_color

    core, folder, _ = plain_run
    assert core.has_heatmap is True
    hm = core.heatmaps(0).cpu().numpy()
    drawn = 0
    for c in (1, 5, 3):   # a right camera, a left (mirrored) camera, the front camera
        blob = open(os.path.join(folder, f"camera_{c}_img_0.jpg"), "rb").read()
        luma = jpeg.decode_luma([blob], 960, 480, device=cuda)[0].cpu().numpy()
        pairs = heatmap_planes(c, camera_ordering=core.camera_ordering)
        ref = ho.overlay_view(luma, hm[c], [p for p, _ in pairs], [plane_color(j) for _, j in pairs], camera_is_flipped(c, core.camera_ordering))
        got = core.plot_heatmap(c, 0)
        assert isinstance(got, np.ndarray) and got.shape == (480, 960, 3) and got.dtype == np.uint8 and np.array_equal(got, ref)
        grey = np.repeat(luma[:, :, None], 3, axis=2)
        if c == 3:
            assert np.array_equal(got, grey)
        drawn += int((got != grey).any(axis=2).sum())
    print(f"pixels tinted on cameras 1 and 5: {drawn}; heat-map range {hm.min():.4g} .. {hm.max():.4g}")
    assert drawn > 0   # the comparison is not one of grey images
    # joints=[j] draws that joint's plane alone: joint 24 is plane 5 of the left cameras; a joint the camera does not fill draws nothing
    blob = open(os.path.join(folder, "camera_5_img_0.jpg"), "rb").read()
    luma = jpeg.decode_luma([blob], 960, 480, device=cuda)[0].cpu().numpy()
    assert np.array_equal(core.plot_heatmap(5, 0, joints=[24]), ho.overlay_view(luma, hm[5], [5], [plane_color(24)], True))
    assert np.array_equal(core.plot_heatmap(5, 0, joints=[5]), np.repeat(luma[:, :, None], 3, axis=2))
    assert np.array_equal(core.plot_heatmap(5, 0, joints=[24], gain=4.0), ho.overlay_view(luma, hm[5], [5], [plane_color(24)], True, gain=4.0))


def test_cli_writes_the_heatmap_video(plain_run, cuda, tmp_path, golden_dir, monkeypatch):
    """`df3d-cli INPUT -n 2 --video-heatmap`: video_heatmap_<folder> with one 2 x 3 grid frame per image, the result pickle what a run
    without the flag writes; the flag alone with --skip-pose-estimation works too."""
    from deepfly3d_amd import cli, jpeg, video
    from deepfly3d_amd.config import config

    core, _, baseline = plain_run
    config.pop("image_shape", None)
    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    folder = _copy_images(golden_dir, str(tmp_path / "images"))
    assert cli.main([folder, "-n", "2", "--video-heatmap", "--output-fps", "12"]) == 0
    out_dir = folder + "_df3d"
    found = [f for f in os.listdir(out_dir) if f.startswith("video_heatmap_")]
    assert len(found) == 1 and not [f for f in os.listdir(out_dir) if f.startswith("video_pose")]
    path = os.path.join(out_dir, found[0])
    assert os.path.splitext(path)[0] == os.path.join(out_dir, "video_heatmap_" + folder.replace("/", "_")) and os.path.getsize(path) > 10000
    assert _result_bytes(folder) == baseline
    if path.endswith(".avi"):
        frames = video.read_mjpeg_avi(path)
        assert len(frames) == 2 and frames[0].shape == (960, 2880, 3)
        blobs = [open(os.path.join(folder, f"camera_{c}_img_0.jpg"), "rb").read() for c in video.GRID_CAMERAS]
        luma = jpeg.decode_luma(blobs, 960, 480, device=cuda)
        hm6 = core.heatmaps(0)[list(video.GRID_CAMERAS)].contiguous()
        ref = video.FrameRenderer(480, 960, 38, cuda).heatmap_grid(luma, hm6, core.camera_ordering).cpu().numpy()
        mad = np.abs(frames[0].astype(np.int32) - ref.astype(np.int32)).mean()
        print(f"first frame against FrameRenderer.heatmap_grid: mean absolute difference {mad:.3f}")
        assert mad < 3.0   # JPEG loss, the bound of the pose-2d video test
    os.remove(path)
    assert cli.main([folder, "-n", "2", "--skip-pose-estimation", "--video-heatmap", "--output-fps", "12"]) == 0
    assert os.path.getsize(path) > 10000
    # the flag needs images and weights only: on a folder without an earlier result it draws, and writes no result
    config.pop("image_shape", None)
    fresh = _copy_images(golden_dir, str(tmp_path / "fresh" / "images"))
    assert cli.main([fresh, "-n", "2", "--skip-pose-estimation", "--video-heatmap"]) == 0
    made = os.listdir(fresh + "_df3d")
    assert [f for f in made if f.startswith("video_heatmap_")] and not [f for f in made if f.startswith("df3d_result")]
    config.pop("image_shape", None)
