"""CPU tests of the tracking of the 2-D detections: the oracle against brute force, the planted distractor, and the
refusals of ops, Core and the command line."""
import dataclasses
import os
import pickle
import re

import numpy as np
import pytest
import torch

import track_cases as tc
import track_oracle as to

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("K", [1, 2, 3])
def test_the_oracle_is_brute_force(K):
    """Every path of tiny tie-heavy cases: the minimum, and among the minimal paths the one whose reversed sequence is lexicographically
    smallest (equal costs are the rule on these inputs; test_reversed_lexicographic_ties_by_hand states the rule on its own)."""
    for seed in range(12):
        T = 1 + seed % 6
        count, pts, val = tc.tie_heavy(100 * K + seed, 1, T, 4, K)
        choice, cost = to.solve(count, pts, val, tc.IMAGE_HW)
        want_choice, want_cost = to.brute_force(count, pts, val, tc.IMAGE_HW)
        assert np.array_equal(cost, want_cost) and np.array_equal(choice, want_choice), (K, seed)
        assert choice.dtype == np.int32 and cost.dtype == np.int64 and choice.shape == (1, T, 4) and cost.shape == (1, 4)
        assert np.all(choice[0][to.slots(count, pts, val, tc.IMAGE_HW)[1]] == 0)   # placeholder frames
    assert np.all(to.solve(*tc.tie_heavy(5, 1, 4, 2, 1), tc.IMAGE_HW)[0] == 0)   # one slot: nothing to choose


def test_reversed_lexicographic_ties_by_hand():
    """Two slots at one place with one value in every frame: all 2^T paths cost 0, and the rule picks slot 0 throughout.  With slot 0 of
    the middle frame made worse, the path avoids it there alone."""
    T = 3
    count = np.full((1, T, 1), 2, np.int32)
    pts = np.full((1, T, 1, 2, 2), 0.25, np.float32)
    val = np.full((1, T, 1, 2), 0.5, np.float32)
    choice, cost = to.solve(count, pts, val, tc.IMAGE_HW)
    assert cost[0, 0] == 0 and choice[0, :, 0].tolist() == [0, 0, 0]
    val[0, 1, 0, 0] = 0.25
    choice, cost = to.solve(count, pts, val, tc.IMAGE_HW)
    assert cost[0, 0] == 0 and choice[0, :, 0].tolist() == [0, 1, 0]
    assert np.array_equal(choice, to.brute_force(count, pts, val, tc.IMAGE_HW)[0])


def test_costs_are_quantised_as_written():
    count = np.array([[[2]], [[2]]], np.int32).reshape(1, 2, 1)
    pts = np.array([[0.5, 0.5], [0.25, 0.25], [0.5, 0.5 + 3.0 / 960.0], [0.0, 0.0]], np.float32).reshape(1, 2, 1, 2, 2)
    val = np.array([[0.9, 0.2], [0.7, 0.65]], np.float32).reshape(1, 2, 1, 2)
    valid, placeholder, rows, cols, qu = to.slots(count, pts, val, tc.IMAGE_HW, w_value=2.0)
    gap = float(np.float32(0.9)) - float(np.float32(0.2))
    assert qu[0, 0].tolist() == [0, int(np.rint(2.0 * gap * 2.0 ** 20))]
    qd = to.pair_costs(valid, placeholder, rows, cols, 1, 2, tau=30.0, w_motion=3.0)[0, 0]
    dc = float(np.float32(0.5 + 3.0 / 960.0)) * 960.0 - 480.0
    assert qd[0, 0] == int(np.rint(3.0 * (dc * dc) / 900.0 * 2.0 ** 20)) and qd[1, 0] == int(np.rint(3.0 * 900.0 / 900.0 * 2.0 ** 20))
    assert to.INF == 2 ** 61 and to.quantise(0.5).dtype == np.int64
    # a frame without a valid slot: slot 0 alone, free, and w_m to and from it
    count[0, 1, 0] = 0
    valid, placeholder, rows, cols, qu = to.slots(count, pts, val, tc.IMAGE_HW)
    assert placeholder[1, 0] and valid[1, 0].tolist() == [True, False] and qu[1, 0].tolist() == [0, to.INF]
    assert to.pair_costs(valid, placeholder, rows, cols, 1, 2, w_motion=0.75)[0, 0, :, 0].tolist() == [int(0.75 * 2 ** 20)] * 2


def test_the_planted_distractor():
    """The condition the case has to meet, then the claim: the arg-max is wrong in at least a fifth of the frames, the tracked path in none."""
    count, pts, val, truth = tc.planted()
    T = truth.shape[1]
    assert T == 200 and int((truth != 0).sum()) >= T // 5
    choice, cost = to.solve(count, pts, val, tc.IMAGE_HW)
    assert int((choice != truth).sum()) == 0
    assert 0 < cost[0, 0] < T * 2 ** 20


def test_without_a_motion_term_every_choice_is_the_arg_max():
    count, pts, val, _ = tc.planted(seed=11, T=60)
    choice, cost = to.solve(count, pts, val, tc.IMAGE_HW, w_motion=0.0)
    assert not choice.any() and not cost.any()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_config_and_oracle_defaults_agree():
    from deepfly3d_amd import config as cfg

    assert cfg.TRACK_DEFAULTS == {"tau": to.TAU, "w_motion": to.W_MOTION, "w_value": to.W_VALUE, "block_frames": to.BLOCK_FRAMES}
    assert (to.TAU, to.W_MOTION, to.W_VALUE, to.BLOCK_FRAMES) == (30.0, 1.0, 1.0, 256) and cfg.TRACK_DEFAULTS["tau"] == cfg.PICTORIAL_DEFAULTS["tau"]
    assert cfg.TRACK_WEIGHT_MAX == 1024.0 and cfg.TRACK_BLOCK_FRAMES_RANGE == (1, 4096) and cfg.TRACK_NUM_PEAKS_RANGE == (1, 16)


def test_ops_refusals():
    from deepfly3d_amd import ops

    assert ops.track_params() == (30.0, 1.0, 1.0, 256) and ops.track_params(7, 0, 1024, 1) == (7.0, 0.0, 1024.0, 1)
    assert ops.track_params(block_frames=4096)[3] == 4096
    for tau in (0.0, -30.0, NAN, INF):
        with pytest.raises(ValueError, match="tau must be finite and > 0"):
            ops.track_params(tau=tau)
    for name in ("w_motion", "w_value"):
        for w in (-0.5, 1024.5, NAN, INF):
            with pytest.raises(ValueError, match=rf"{name} must be finite and in \[0, 1024\]"):
                ops.track_params(**{name: w})
    for name in ("tau", "w_motion", "w_value"):
        for v in ("1", True, [1.0]):
            with pytest.raises(ValueError, match=f"{name} must be a number"):
                ops.track_params(**{name: v})
    for b in (0, 4097, -1, 256.0, True, "256"):
        with pytest.raises(ValueError, match=r"block_frames must be an integer in \[1, 4096\]"):
            ops.track_params(block_frames=b)
    count, pts, val = (torch.from_numpy(a) for a in tc.tie_heavy(0, 2, 4, 3, 5))
    with pytest.raises(ValueError, match="peak_count must be a contiguous torch.int32 CUDA tensor"):
        ops.track_peaks(count, pts, val, [960, 480])
    with pytest.raises(ValueError, match="tau must be finite"):   # the parameters come first
        ops.track_peaks(count, pts, val, [960, 480], tau=0.0)
    with pytest.raises(ValueError, match="points2d must be a contiguous torch.float64 CUDA tensor"):
        ops.tracked_points2d(torch.zeros((7, 4, 38, 2), dtype=torch.float64), range(7), pts, torch.zeros((7, 4, 19), dtype=torch.int32))
    assert [f.name for f in dataclasses.fields(ops.TrackResult)] == ["choice", "cost", "params"]
    r = ops.TrackResult(None, torch.tensor([[3 << 19]]), ())
    assert r.cost_float.dtype == torch.float64 and float(r.cost_float[0, 0]) == 1.5


def test_command_line_refusals(capsys):
    from deepfly3d_amd import cli

    for argv, message in ((["x", "--track-tau", "20"], "--track-tau sets a parameter of --track-2d: it needs --track-2d"),
                          (["x", "--track-motion", "2"], "--track-motion sets a parameter of --track-2d: it needs --track-2d"),
                          (["x", "--track-value", "2"], "--track-value sets a parameter of --track-2d: it needs --track-2d"),
                          (["x", "--track-2d", "--skip-pose-estimation"], "--track-2d needs the heat-map peaks of this run's pose estimation"),
                          (["x", "--track-2d", "--auto-correct"], "--track-2d and --auto-correct both start from the arg-max detections"),
                          (["x", "--track-2d", "--track-tau", "0"], "tau must be finite and > 0"),
                          (["x", "--track-2d", "--track-tau", "nan"], "tau must be finite and > 0"),
                          (["x", "--track-2d", "--track-motion=-1"], r"w_motion must be finite and in \[0, 1024\]"),
                          (["x", "--track-2d", "--track-value", "1025"], r"w_value must be finite and in \[0, 1024\]"),
                          (["x", "--track-2d", "--track-value", "much"], "invalid float value")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err), argv
    args = cli.parse_cli_args(["x", "--track-2d", "--track-tau", "12.5", "--track-motion", "0", "--track-value", "3", "--gait"])
    assert args.track_2d and (args.track_tau, args.track_motion, args.track_value) == (12.5, 0.0, 3.0)
    args = cli.parse_cli_args(["x"])
    assert not args.track_2d and args.track_tau is None and args.track_motion is None and args.track_value is None
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for option in ("--track-2d", "--track-tau PX", "--track-motion W", "--track-value W"):
        assert option in text
    assert "guesses that nobody has measured on a recording" in text


def _one_frame_core(tmp_path, golden_dir):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    folder = tmp_path / "images"   # one frame per camera and no earlier result
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    config.pop("image_shape", None)
    core = Core(str(folder), str(folder) + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    config.pop("image_shape", None)
    return core


def test_core_refusals(tmp_path, golden_dir):
    core = _one_frame_core(tmp_path, golden_dir)
    with pytest.raises(RuntimeError, match=r"track_detections needs the heat-map peaks of this recording: run pose2d_estimation\(num_peaks=K\) first"):
        core.track_detections()
    with pytest.raises(TypeError, match=r"track_detections: unknown parameters \['num_peaks', 'w_bone'\]"):
        core.track_detections(w_bone=1.0, num_peaks=10)
    with pytest.raises(ValueError, match="tau must be finite"):   # before the peaks are asked for
        core.track_detections(tau=-1.0)
    with pytest.raises(ValueError, match="block_frames must be an integer"):
        core.track_detections(block_frames=5000)
    core.points2d = np.zeros((7, 3, 38, 2))
    core.peaks = tuple(tc.tie_heavy(0, 7, 2, 19, 4))   # the peaks of another recording: two frames, not three
    with pytest.raises(RuntimeError, match="track_detections needs the heat-map peaks of this recording"):
        core.track_detections()
    assert core._track is None and core.points2d_argmax is None and not core.points2d.any()


def test_the_keys_follow_points2d_argmax(tmp_path, golden_dir, monkeypatch):
    """Core.track_detections and save with the device solve replaced by the oracle: what is stored, where, and that the arg-max detections
    survive a second call and a later pose estimation forgets the tracking."""
    from deepfly3d_amd import _native, ops
    from oracle import geometry as og

    T, K, order = 12, 4, list(range(7))
    core = _one_frame_core(tmp_path, golden_dir)
    count, pts, val = tc.tie_heavy(21, 7, T, 19, K, dirty=False)
    count[:] = np.maximum(count, 1)
    pts[..., 0] += (np.arange(K) / 1024.0).astype(np.float32)   # no two slots of a frame at one place: a moved detection differs
    core.device, core.num_images = "cpu", T
    core.peaks = (count, pts, val)
    core.points2d = og.relayout_19_to_38(pts[:, :, :, 0], order)
    core.conf = np.zeros((7, T, 19, 1), np.float32)
    calls = []

    def track_peaks(peak_count, peak_pts, peak_val, image_shape, tau=None, w_motion=None, w_value=None, block_frames=None):
        p = ops.track_params(tau, w_motion, w_value, block_frames)
        calls.append(p)
        choice, cost = to.solve(peak_count.numpy(), peak_pts.numpy(), peak_val.numpy(), image_shape[::-1], *p[:3])
        return ops.TrackResult(torch.from_numpy(choice), torch.from_numpy(cost), p)

    def tracked_points2d(points2d, camera_ordering, peak_pts, choice):
        chosen = np.take_along_axis(peak_pts.numpy(), choice.numpy()[..., None, None].astype(np.int64), axis=3)[:, :, :, 0]
        moved = og.relayout_19_to_38(np.repeat((choice.numpy() != 0)[..., None], 2, axis=-1).astype(np.float32), camera_ordering)[..., 0] != 0
        return torch.from_numpy(np.where(moved[..., None], og.relayout_19_to_38(chosen, camera_ordering), points2d.numpy()))

    monkeypatch.setattr(_native, "require_gpu", lambda: 1)
    monkeypatch.setattr(ops, "track_peaks", track_peaks)
    monkeypatch.setattr(ops, "tracked_points2d", tracked_points2d)
    argmax = core.points2d.copy()
    core.save()
    with open(core.save_path, "rb") as f:
        plain = pickle.load(f)
    assert list(plain) == ["points2d", "camera_ordering", "heatmap_confidence"]

    core.track_detections(tau=20.0, w_value=0.5)
    assert calls == [(20.0, 1.0, 0.5, 256)] and core._corrected
    core.track_detections(tau=20.0, w_value=0.5)   # again: from the arg-max detections, not from its own result
    core.save()
    with open(core.save_path, "rb") as f:
        saved = pickle.load(f)
    assert list(saved) == ["points2d", "camera_ordering", "heatmap_confidence", "points2d_argmax", "track_choice", "track_cost", "track_params"]
    choice, cost = to.solve(count, pts, val, (480, 960), 20.0, 1.0, 0.5)
    assert saved["track_choice"].dtype == np.int8 and saved["track_choice"].shape == (7, T, 19) and np.array_equal(saved["track_choice"], choice)
    assert saved["track_cost"].dtype == np.float64 and np.array_equal(saved["track_cost"], cost / 2.0 ** 20)
    assert saved["track_params"].tolist() == [20.0, 1.0, 0.5]
    assert np.array_equal(saved["points2d_argmax"], argmax) and choice.any()
    moved = og.relayout_19_to_38(np.repeat((choice != 0)[..., None], 2, axis=-1).astype(np.float32), order)[..., 0] != 0
    assert np.array_equal((saved["points2d"] != argmax).any(axis=-1), moved)
    assert np.array_equal(saved["points2d"], core.points2d) and np.array_equal(plain["points2d"], argmax)
