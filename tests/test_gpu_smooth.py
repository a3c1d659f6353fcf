"""GPU tests of the temporal smoothing of 2-D detections and of the manual correction round trip:
df3d_smooth_pose2d against outputs of the reference's `smooth_pose2d` (tests/golden/smooth_golden.npz) and against the float64
oracle tests/smooth_oracle.py on a seeded sweep with poisoned outputs; non-finite samples; T = 0; ops.filter_batch_2d bit for bit;
Core.smooth_points2d and its cache, plot_2d(smooth=True), `df3d-cli --video-2d [--smooth-2d]`; move_joint -> next_error -> save()."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import smooth_oracle as so
from test_gpu_reproj import HW, ORDER, _folder, _resumed_core

pytestmark = pytest.mark.gpu

# |out - ref| in pixels: a window sum of at most 57 folded taps on values <= 1 000 px in float64 is bounded by 57 * 2^-53 * 1000 = 6e-12;
# 1e-10 leaves a margin for the summation order
ATOL = 1e-10
NEAR = 1e-9          # an output whose reference deviation lies this near std_thr may take either branch ...
NEAR_SHARE = 1e-3    # ... and such outputs are at most 0.1 % of a case
TILE = 64            # frames per block of smooth_kernel (csrc/smooth.hip)


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(cuda)


def _check(got, inp, ref_out, ref_std, window, thr, what, ws=None, wk=None):
    """got against the reference output; where the reference deviation is within NEAR of thr either branch's value is accepted."""
    flat = inp.reshape(inp.shape[:-2] + (-1,)) if inp.ndim >= 3 and inp.shape[-1] == 2 else inp
    smoothed, _ = so.smooth(flat, window, np.inf, ws, wk)
    kept, _ = so.smooth(flat, window, 0.0, ws, wk)
    got, ref_out, ref_std = (np.asarray(a).reshape(flat.shape) for a in (got, ref_out, ref_std))
    with np.errstate(invalid="ignore"):
        near = np.abs(ref_std - thr) <= NEAR
        ok = np.abs(got - ref_out) <= ATOL
        either = (np.abs(got - smoothed) <= ATOL) | (np.abs(got - kept) <= ATOL)
    ok |= (got == ref_out) | (np.isnan(got) & np.isnan(ref_out))      # infinities and NaNs pass through as they are
    worst = np.nanmax(np.where(near | ~np.isfinite(ref_out), 0.0, np.abs(got - ref_out))) if got.size else 0.0
    print(f"{what}: max |out - ref| = {worst:.3e} px, threshold cells {int(near.sum())} of {near.size}")
    assert near.sum() <= NEAR_SHARE * max(near.size, 1), what
    assert np.all(np.where(near, either | ok, ok)), (what, worst)


# ------------------------------------------------------------------------------------------------------------------ kernel
def test_fixture_lengths_match_the_reference_and_the_oracle(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops

    g = np.load(f"{golden_dir}/smooth_golden.npz")
    for T in (1, 2, 9, 21, 400):
        inp, out, std = g[f"inp_{T}"], g[f"out_{T}"], g[f"std_{T}"]
        got = ops.smooth_pose2d(_dev(cuda, inp)).cpu().numpy()
        assert got.shape == inp.shape
        _check(got, inp, out, std, 20, 5.0, f"reference T={T}")
        o_out, o_std = so.smooth(inp.reshape(T, 76), 20, 5.0)
        _check(got, inp, o_out, o_std, 20, 5.0, f"oracle T={T}")
    # all seven cameras in one launch: the 400-frame case seven times, each camera shifted
    inp = np.stack([g["inp_400"] + 3.0 * c * (g["inp_400"] != 0) for c in range(7)])
    got = ops.smooth_pose2d(_dev(cuda, inp)).cpu().numpy()
    o_out, o_std = so.smooth(inp.reshape(7, 400, 76), 20, 5.0)
    _check(got, inp, o_out, o_std, 20, 5.0, "oracle 7 x 400")
    assert np.array_equal(got[0], ops.smooth_pose2d(_dev(cuda, inp[0])).cpu().numpy())


def _raw(lib, pts, C, T, nch, window, thr, ws, wk):
    out = torch.full_like(pts, float("nan"))      # poisoned: a cell the kernel does not write stays NaN
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.df3d_smooth_pose2d(pts.data_ptr(), C, T, nch, window, thr, ws.ctypes.data_as(dp), wk.ctypes.data_as(dp), out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("window", [2, 20, 64])
@pytest.mark.parametrize("nch", [2, 76, 128])
@pytest.mark.parametrize("C", [1, 7, 8])
def test_sweep_with_poisoned_outputs(native_lib, cuda, C, nch, window):
    from deepfly3d_amd import ops

    rng = np.random.default_rng(1000 * C + 10 * nch + window)
    ws, wk = ops.gaussian_window_taps(window, 7.0), ops.gaussian_window_taps(window, 0.1)
    for T in (TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        x = rng.uniform(50.0, 900.0, size=(C, 1, nch)) + np.cumsum(rng.normal(0.0, 1.5, size=(C, T, nch)), axis=0 + 1)
        x[:, T // 3: 2 * T // 3] += rng.normal(0.0, 12.0, size=x[:, T // 3: 2 * T // 3].shape)   # both branches
        x[:, :, 0] = 0.0
        got = _raw(native_lib, _dev(cuda, x), C, T, nch, window, 5.0, ws, wk)
        assert not np.isnan(got).any(), "unwritten cells"
        want, std = so.smooth(x, window, 5.0, ws, wk)
        assert (std >= 5.0).any() and (std < 5.0).any()
        _check(got, x, want, std, window, 5.0, f"C={C} nch={nch} W={window} T={T}", ws, wk)


def test_general_keep_taps_and_thresholds(native_lib, cuda):
    """The two coefficient vectors are arguments: a keep filter with several taps, thr = 0 (never smooth) and thr = inf (always)."""
    from deepfly3d_amd import ops

    rng = np.random.default_rng(77)
    x = 400.0 + np.cumsum(rng.normal(0.0, 2.5, size=(2, 150, 6)), axis=1)
    ws, wk = ops.gaussian_window_taps(20, 7.0), ops.gaussian_window_taps(20, 1.0)
    assert np.count_nonzero(wk) == 9
    for thr in (0.0, 6.0, float("inf")):
        got = _raw(native_lib, _dev(cuda, x), 2, 150, 6, 20, thr, ws, wk)
        want, std = so.smooth(x, 20, thr, ws, wk)
        _check(got, x, want, std, 20, thr, f"keep sigma 1, thr {thr}", ws, wk)


def test_non_finite_samples_pass_through(native_lib, cuda):
    from deepfly3d_amd import ops

    rng = np.random.default_rng(9)
    x = 300.0 + np.cumsum(rng.normal(0.0, 1.0, size=(200, 38, 2)), axis=0)
    clean = ops.smooth_pose2d(_dev(cuda, x)).cpu().numpy()
    y = x.copy()
    y[70, 4, 1], y[130, 20, 0], y[63, 9, 0], y[0, 1, 1], y[199, 2, 0] = np.nan, np.inf, -np.inf, np.nan, np.inf
    got = ops.smooth_pose2d(_dev(cuda, y)).cpu().numpy()
    want = so.smooth_pose2d(y)
    touched = np.zeros(x.shape, dtype=bool)
    for t, j, d in ((70, 4, 1), (130, 20, 0), (63, 9, 0), (0, 1, 1), (199, 2, 0)):
        lo, hi = max(t - 9, 0), min(t + 10, 199)      # the windows t' - 10 .. t' + 9 that hold frame t (all of them at a replicated edge)
        lo, hi = (0, hi) if t == 0 else (lo, 199) if t == 199 else (lo, hi)
        touched[lo:hi + 1, j, d] = True
        assert np.array_equal(got[lo:hi + 1, j, d], y[lo:hi + 1, j, d], equal_nan=True)   # every such window keeps its centre sample
    assert np.array_equal(got[~touched], clean[~touched])                                  # ... and no other output changes at all
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.abs(got[np.isfinite(got)] - want[np.isfinite(want)]).max() <= ATOL


def test_empty_recording_and_argument_errors(native_lib, cuda):
    from deepfly3d_amd import _native, ops

    for shape in ((0, 38, 2), (7, 0, 38, 2), (0, 5, 38, 2)):
        out = ops.smooth_pose2d(torch.zeros(shape, dtype=torch.float64, device=cuda))
        assert tuple(out.shape) == shape and out.dtype == torch.float64 and out.device.type == "cuda"
    x = torch.zeros((3, 38, 2), dtype=torch.float64, device=cuda)
    with pytest.raises(_native.NativeLibraryError, match="window"):
        ops.smooth_pose2d(x, window_size=21)
    with pytest.raises(_native.NativeLibraryError, match="std_thr"):
        ops.smooth_pose2d(x, std_thr=-1.0)
    with pytest.raises(_native.NativeLibraryError, match="C must"):
        ops.smooth_pose2d(torch.zeros((9, 3, 38, 2), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        ops.smooth_pose2d(x.float())
    with pytest.raises(ValueError):
        ops.smooth_pose2d(torch.zeros((3, 38, 3), dtype=torch.float64, device=cuda))
    # validation returns DF3D_EINVAL without a launch: a poisoned output stays poisoned
    out = torch.full((4, 76), float("nan"), dtype=torch.float64, device=cuda)
    taps = np.full(20, 0.05)
    dp = ctypes.POINTER(ctypes.c_double)
    src = torch.ones((4, 76), dtype=torch.float64, device=cuda)
    for C, nch, window, thr in ((0, 76, 20, 5.0), (1, 129, 20, 5.0), (1, 76, 22 + 1, 5.0), (1, 76, 20, float("nan"))):
        rc = native_lib.df3d_smooth_pose2d(src.data_ptr(), C, 4, nch, window, thr, taps.ctypes.data_as(dp), taps.ctypes.data_as(dp), out.data_ptr(), None)
        assert rc == _native.DF3D_EINVAL
    assert native_lib.df3d_smooth_pose2d(src.data_ptr(), 1, 4, 76, 20, 5.0, taps.ctypes.data_as(dp), taps.ctypes.data_as(dp), src.data_ptr(), None) == _native.DF3D_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((src == 1.0).all())
    # leading dimensions: [2, 3, T, J, 2] is six cameras
    rng = np.random.default_rng(4)
    y = 200.0 + np.cumsum(rng.normal(0.0, 1.0, size=(2, 3, 90, 5, 2)), axis=2)
    got = ops.smooth_pose2d(_dev(cuda, y)).cpu().numpy()
    assert np.abs(got - so.smooth_pose2d(y)).max() <= ATOL


def test_filter_batch_2d_bit_exact(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops

    d = np.load(f"{golden_dir}/oneeuro2d_random.npz")
    assert d["inp"].shape == (300, 38, 2)
    got = ops.filter_batch_2d(_dev(cuda, d["inp"])).cpu().numpy()
    assert np.array_equal(got, d["out"])
    assert not np.array_equal(got, ops.oneeuro_filter(_dev(cuda, d["inp"])).cpu().numpy())   # not filter_batch's constants
    assert np.array_equal(ops.filter_batch_2d(_dev(cuda, d["inp"][:1])).cpu().numpy(), d["inp"][:1])


# ------------------------------------------------------------------------------------------------------------------ Core
def test_core_smooth_points2d_cache_and_plot(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    p2 = g3["points2d"].copy()
    cam, t, j = 1, 7, 8
    p2[cam, :, j] = p2[cam, 0, j]           # a joint at rest ...
    p2[cam, t, j, 1] += 15.0 / 960.0       # ... but for a one-frame jump of 15 px: window deviation 15 * sqrt(0.05 * 0.95) = 3.3 < 5, so it is smoothed
    core = _resumed_core(_folder(tmp_path, golden_dir), golden_dir, p2)
    for c in range(7):
        want = ops.smooth_pose2d(_dev(cuda, core.camNet[c].points2d)).cpu().numpy()
        got = core.smooth_points2d(c)
        assert got.shape == (15, 38, 2) and np.array_equal(got, want)
    first = core.camNet._smoothed
    assert not core.smooth_points2d(cam).flags.writeable                      # one array for every caller: handed out read-only
    assert np.shares_memory(core.smooth_points2d(cam), first) and core.camNet._smoothed is first   # kept on the network ...
    assert not np.shares_memory(core.smooth_points2d(cam, refresh=True), first)                    # ... until asked
    assert abs(core.smooth_points2d(cam)[t, j, 1] - core.camNet[cam].points2d[t, j, 1]) > 5.0
    # plot_2d: the default draws the detection, smooth=True the smoothed one; a stored correction wins over both
    raw = core.plot_2d(cam, t)
    assert np.array_equal(raw, core.plot_2d(cam, t, smooth=False)) and np.array_equal(raw, core.camNet[cam].plot_2d(t))
    smooth = core.plot_2d(cam, t, smooth=True)
    assert smooth.shape == raw.shape and not np.array_equal(smooth, raw)
    assert np.array_equal(smooth, core.camNet[cam].plot_2d(t, points2d=core.smooth_points2d(cam)[t]))
    fix = core.camNet[cam].points2d[t].copy()
    fix[j] += [60.0, 60.0]
    core.write_corrections(cam, t, [j], fix)
    fixed = core.plot_2d(cam, t, with_corrections=True, smooth=True)
    assert np.array_equal(fixed, core.plot_2d(cam, t, with_corrections=True)) and not np.array_equal(fixed, smooth)
    assert np.array_equal(core.plot_2d(cam, t, smooth=True), smooth)
    # corrected_points2d_matrix writes the correction into the network: the smoothed points are dropped and follow
    before = core.smooth_points2d(cam).copy()
    core.corrected_points2d_matrix()
    assert core.camNet._smoothed is None
    after = core.smooth_points2d(cam)
    assert not np.array_equal(after, before) and np.array_equal(after, ops.smooth_pose2d(_dev(cuda, core.camNet[cam].points2d)).cpu().numpy())
    # a new network (calibrate_calc) starts without them
    core.calibrate_calc(0, core.max_img_id)
    assert core.camNet._smoothed is None
    config.pop("image_shape", None)


def test_auto_correct_drops_the_smoothed_points(native_lib, cuda, tmp_path, golden_dir):
    import test_gpu_pictorial as tgp

    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    P, hm, _ = tgp._render(golden_dir)
    am, _, _, _, (count, pts, vals) = tgp._run(P, hm, cuda)
    core = _resumed_core(_folder(tmp_path, golden_dir, hm.shape[1]), golden_dir, am.cpu().numpy())
    core.peaks = tuple(x.cpu().numpy() for x in (count, pts, vals))
    assert core.smooth_points2d(0) is not None and core.camNet._smoothed is not None
    core.auto_correct()
    assert core.camNet._smoothed is None
    config.pop("image_shape", None)


def test_cli_video_2d_with_and_without_smoothing(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    """`df3d-cli --skip-pose-estimation --video-2d` on a saved result draws the detections exactly as before (frame for frame what
    the renderer draws from the saved points, through the same encoder); with `--smooth-2d` the frames differ."""
    from deepfly3d_amd import cli, jpeg, video
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    monkeypatch.setattr(video.shutil, "which", lambda name: None)      # Motion-JPEG in AVI: frames that read_mjpeg_avi reads back
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    folder = _folder(tmp_path, golden_dir, 15)
    # the golden detections with 3 px of seeded jitter: quiet joints are smoothed by whole pixels in every frame
    p2 = g3["points2d"] + (g3["points2d"] != 0) * np.random.default_rng(8).normal(0.0, 3.0, size=g3["points2d"].shape) / HW
    core = _resumed_core(folder, golden_dir, p2)
    out_dir, flat = core.output_folder, core.input_folder.replace("/", "_")
    del core
    args = [folder, "--skip-pose-estimation", "--video-2d", "--output-fps", "10", "--order", *[str(c) for c in ORDER]]
    assert cli.main(args) == 0
    path = os.path.join(out_dir, f"video_pose2d_{flat}.avi")
    plain = video.read_mjpeg_avi(path)
    with open(os.path.join(out_dir, f"df3d_result_{flat}.pkl"), "rb") as f:
        saved = pickle.load(f)
    assert np.array_equal(saved["points2d"], p2)
    # as before: the renderer on the saved detections, written by the same encoder
    renderer = video.FrameRenderer(480, 960, 38, cuda)
    blobs = [open(os.path.join(folder, f"camera_{c}_img_0.jpg"), "rb").read() for c in video.GRID_CAMERAS]
    luma = jpeg.decode_luma(blobs, 960, 480, device=cuda)
    writer = video.MjpegAviWriter(str(tmp_path / "expected.avi"), 2880, 960, 10)
    for t in range(15):
        pts = np.stack([saved["points2d"][c, t] * HW for c in video.GRID_CAMERAS])
        writer.write(renderer.grid2d(luma, torch.from_numpy(pts).to(cuda)).cpu().numpy())
    writer.close()
    expected = video.read_mjpeg_avi(str(tmp_path / "expected.avi"))
    assert len(plain) == len(expected) == 15 and all(np.array_equal(a, b) for a, b in zip(plain, expected))
    assert cli.main(args + ["--smooth-2d"]) == 0
    smooth = video.read_mjpeg_avi(path)
    assert len(smooth) == 15 and sum(not np.array_equal(a, b) for a, b in zip(smooth, plain)) >= 10
    with pytest.raises(SystemExit):
        cli.main([folder, "--skip-pose-estimation", "--video-3d", "--smooth-2d"])
    config.pop("image_shape", None)


def test_move_joint_round_trip_reaches_the_error_search_and_save(native_lib, cuda, tmp_path, golden_dir):
    """Plant a 120 px error, find it with next_error, move the joint back with move_joint: the frame's joint is no longer flagged
    and save() triangulates it where the unperturbed recording has it (atol 1e-8, the bar of the resumed golden run)."""
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    folder = _folder(tmp_path, golden_dir)
    clean = _resumed_core(folder, golden_dir, g3["points2d"])
    clean.save()
    with open(clean.save_path, "rb") as f:
        base = pickle.load(f)
    flagged = [t for t in range(15) if clean.next_error(t - 1) == t]
    cam, j = 1, 8
    t = next(t for t in range(3, 15) if t not in flagged)
    true_px = clean.camNet[cam].points2d[t, j].copy()
    p2 = g3["points2d"].copy()
    p2[cam, t, j, 1] += 120.0 / 960.0
    core = _resumed_core(folder, golden_dir, p2)
    assert core.joint_has_error(t, j) and core.next_error(t - 1) == t
    assert core.nearest_joint(cam, t, true_px[0], true_px[1] + 120.0) == j
    core.move_joint(cam, t, j, true_px[0], true_px[1])
    assert core.db.read_modified_joints(cam, t) == [j] and core.joint_has_error(t, j)   # stored, not yet in the camera network
    core.corrected_points2d_matrix()
    assert np.abs(core.camNet[cam].points2d[t] - clean.camNet[cam].points2d[t]).max() < 1e-9
    assert not core.joint_has_error(t, j) and core.next_error(t - 1) == clean.next_error(t - 1) != t
    core.save()
    with open(core.save_path, "rb") as f:
        fixed = pickle.load(f)
    np.testing.assert_allclose(fixed["points3d_wo_procrustes"][t, j], base["points3d_wo_procrustes"][t, j], atol=1e-8)
    np.testing.assert_allclose(fixed["points3d_wo_procrustes"], base["points3d_wo_procrustes"], atol=1e-8)
    np.testing.assert_allclose(fixed["points3d"][t, j], base["points3d"][t, j], atol=1e-8)
    config.pop("image_shape", None)
