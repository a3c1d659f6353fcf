"""CPU tests of the gait model: the oracle against hand-written cases and against its own invariants, the
planted walker recovered by the oracle alone, the numpy restatement of the coupling kernel's form inside the coupling's bar, and
every refusal of ops, Core and the command line that comes before the device."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402
import joint_angles_oracle as jo  # noqa: E402

NAN = float("nan")


def _column(values, leg=0):
    u = np.full((len(values), 6), 2.5)   # in band
    u[:, leg] = values
    return u


# ------------------------------------------------------------------------------------------------------------------ the state rule
def test_state_rule_by_hand():
    on, off = go.ON, go.OFF
    cases = [
        # a leading in-band run stays unknown; the thresholds themselves are in band
        ([2.0, on, off, 6.0, on, 3.0, off, -1.0, off, on, 5.5], [-1, -1, -1, 1, 1, 1, 1, 0, 0, 0, 1]),
        # a NaN in the middle: unknown persists through the in-band samples until a decisive one
        ([6.0, 1.0, NAN, 1.0, 4.0, -0.5, 2.0, NAN, 7.0], [1, 1, -1, -1, -1, 0, 0, -1, 1]),
        # infinities decide
        ([np.inf, 1.0, -np.inf, 1.0], [1, 1, 0, 0]),
        # never decisive
        ([1.0, 2.0, 3.0, 4.0], [-1, -1, -1, -1]),
        # alternating every frame
        ([6.0, -1.0, 6.0, -1.0, 6.0], [1, 0, 1, 0, 1]),
    ]
    for values, want in cases:
        got = go.states_of(_column(values, 3))
        assert got.dtype == np.int32 and got[:, 3].tolist() == want, values
        assert np.all(got[:, [0, 1, 2, 4, 5]] == -1)
    assert go.states_of(_column([1.0, 3.0, 1.0]), on=2.0, off=1.5)[:, 0].tolist() == [0, 1, 0]
    assert go.states_of(np.zeros((0, 6))).shape == (0, 6)


def test_one_frame_is_all_unknown():
    X = go.random_poses(1)
    r = go.gait(X, 100.0, np.eye(3))
    assert np.all(np.isnan(r["vel"])) and np.all(r["states"] == -1) and np.all(np.isfinite(r["tip"]))
    assert r["steps"].shape == (0, 4) and np.all(np.isnan(r["phase"])) and r["pattern"].tolist() == [-1]
    assert np.all(np.isnan(r["coupling"])) and not r["coupling_count"].any() and not r["pattern_histogram"].any()
    assert r["state_counts"].tolist() == [[1, 0, 0]] * 6


def test_window_clipping():
    T, w, fps = 9, 3, 50.0
    rng = np.random.default_rng(0)
    X = rng.normal(size=(T, 38, 3))
    tip, vel = go.tip_kinematics(X, fps, np.eye(3), w)
    a, b = go.window(T, w)
    assert a.tolist() == [0, 0, 0, 0, 1, 2, 3, 4, 5] and b.tolist() == [3, 4, 5, 6, 7, 8, 8, 8, 8]
    for t in range(T):
        for leg in range(6):
            d = X[b[t], go.TIPS[leg]] - X[a[t], go.TIPS[leg]]
            sign = -1.0 if leg >= 3 else 1.0
            want = np.array([d[0], sign * d[1], d[2]]) * (fps / (b[t] - a[t]))
            assert np.array_equal(vel[t, leg], want), (t, leg)   # the identity frame: products with 1 and sums with 0 are exact
            r = X[t, go.TIPS[leg]] - X[t, go.COXAE[leg]]
            assert np.array_equal(tip[t, leg], [r[0], sign * r[1], r[2]])
    # the tip at t itself need not exist for the velocity; at a window's end it must
    X[4, go.TIPS[2]] = 0.0
    tip, vel = go.tip_kinematics(X, fps, np.eye(3), w)
    assert np.all(np.isnan(tip[4, 2])) and np.all(np.isfinite(vel[4, 2]))
    gone = [t for t in range(T) if a[t] == 4 or b[t] == 4]
    assert gone == [1, 7] and np.all(np.isnan(vel[gone, 2])) and np.isnan(vel[:, 2, 0]).sum() == 2
    assert np.isfinite(vel[:, [0, 1, 3, 4, 5]]).all()
    # a missing coxa takes the tip's position, not its velocity; a non-finite frame takes both
    X[5, go.COXAE[0]] = 0.0
    F = np.broadcast_to(np.eye(3), (T, 3, 3)).copy()
    F[6, 1, 1] = np.inf
    tip, vel = go.tip_kinematics(X, fps, F, w)
    assert np.all(np.isnan(tip[5, 0])) and np.all(np.isfinite(vel[5, 0]))
    assert np.all(np.isnan(tip[6])) and np.all(np.isnan(vel[6])) and np.all(np.isfinite(vel[5, [0, 1, 3, 4, 5]]))


# ------------------------------------------------------------------------------------------------------------------ steps, phase
def _states(rows):
    """[T, 6] from six strings of u (unknown), s (stance), w (swing)."""
    return np.array([["usw".index(c) - 1 for c in row] for row in rows], dtype=np.int32).T.copy()


def test_steps_and_phase_by_hand():
    rows = ["swwsswwwsssws",    # lift-offs at 1, 5, 11: two steps
            "sswwsswuwssww",    # lift-offs at 2, 6, 11: an unknown frame inside the second cycle drops it and leaves its neighbour
            "wwsswwsswwssw",    # starts in swing: lift-offs at 4, 8, 12
            "uuuuuuuuuuuuu", "sssssssssssss",
            "swswswswswsws"]    # alternates every frame: lift-offs at 1, 3, ..., 11
    s = _states(rows)
    T = s.shape[0]
    tip = np.zeros((T, 6, 3))
    tip[:, :, 0] = np.arange(T)[:, None] * np.arange(1, 7)[None, :]
    tip[6, 2, 0] = NAN
    fps = 40.0
    steps, metrics = go.steps_of(s, tip, fps)
    want = [(0, 1, 3, 5), (0, 5, 8, 11), (1, 2, 4, 6), (2, 4, 6, 8), (2, 8, 10, 12)] + [(5, t, t + 1, t + 2) for t in range(1, 11, 2)]
    assert steps.dtype == np.int64 and steps.tolist() == [list(row) for row in want]
    assert steps.tolist() == sorted(steps.tolist())   # ordered by (leg, t0)
    lift, touch = go.events(s)
    for leg, t0, t1, t2 in steps:
        assert touch[t0:t2 + 1, leg].sum() == 1 and touch[t1, leg] and lift[t0, leg] and lift[t2, leg] and not lift[t0 + 1:t2, leg].any()
    assert np.array_equal(metrics[:, 0], (steps[:, 2] - steps[:, 1]) / fps) and np.array_equal(metrics[:, 1], (steps[:, 3] - steps[:, 2]) / fps)
    stride = metrics[:, 2]
    assert stride[0] == 2.0 and stride[2] == 4.0 and np.isnan(stride[3]) and stride[4] == 6.0 and np.isnan(stride).sum() == 1
    phase = go.phase_of(s)
    for leg in range(6):
        inside = np.zeros(T, dtype=bool)
        for _, t0, _, t2 in steps[steps[:, 0] == leg]:
            p = phase[t0:t2, leg]
            assert p[0] == 0.0 and np.all(np.diff(p) > 0) and p[-1] < 1.0
            assert np.array_equal(p, np.arange(t2 - t0) / (t2 - t0))
            inside[t0:t2] = True
        assert np.array_equal(np.isfinite(phase[:, leg]), inside)
    assert np.isnan(phase[6:11, 1]).all() and np.isnan(phase[:, 3:5]).all()


def test_coupling_and_patterns_invariants():
    rng = np.random.default_rng(2)
    u = go.u_cases(3000, seed=2)
    u[:, 3] = np.where(rng.random(3000) < 0.5, 8.0, -3.0)   # a leg that does step
    s = go.states_of(u)
    phase = go.phase_of(s)
    mean, count = go.coupling(phase)
    finite = np.isfinite(phase)
    for i in range(6):
        n = int(finite[:, i].sum())
        assert count[i, i] == n
        if n:
            assert mean[i, i].tolist() == [1.0, 0.0]
        else:
            assert np.isnan(mean[i, i]).all()
        for j in range(6):
            assert count[i, j] == count[j, i] == int((finite[:, i] & finite[:, j]).sum())
            if count[i, j]:
                assert abs(mean[i, j, 0] - mean[j, i, 0]) < 1e-15 and abs(mean[i, j, 1] + mean[j, i, 1]) < 1e-15
                assert np.hypot(*mean[i, j]) <= 1.0 + 1e-15
    assert count[0, 0] > 100 and count[3, 3] > 100 and count[4, 4] > 2900   # the cases do step
    pattern, histogram, counts = go.patterns(s)
    assert pattern.dtype == np.int32 and histogram.dtype == np.int64 and counts.dtype == np.int64
    assert histogram.sum() == (pattern >= 0).sum() and np.all(counts.sum(axis=1) == 3000)
    assert np.array_equal(pattern == -1, np.any(s == -1, axis=1))
    known = pattern >= 0
    for leg in range(6):
        assert np.array_equal((pattern[known] >> leg) & 1, (s[known, leg] == 1).astype(np.int32))
    s2 = _states(["wsw", "sws", "wsw", "sws", "wsw", "swu"])
    assert go.patterns(s2)[0].tolist() == [21, 42, -1] and go.TRIPODS == (21, 42)


def test_the_kernels_coupling_form_is_inside_the_bar():
    """The product form in the kernel's order of summation against the model's cos and sin of the difference, summed exactly."""
    worst = 0.0
    for T, seed in ((1, 0), (300, 1), (2047, 2), (2048, 3), (2049, 4), (20000, 5)):
        rng = np.random.default_rng(seed)
        phase = rng.random((T, 6))
        phase[rng.random((T, 6)) < 0.2] = NAN
        phase[:, 5] = NAN if T == 300 else phase[:, 5]
        want, count = go.coupling(phase)
        got, count2 = go.coupling_kernel_form(phase)
        assert np.array_equal(count, count2) and np.array_equal(np.isnan(want), np.isnan(got))
        fraction = np.abs(got - want) / go.coupling_bar(count)[..., None]
        worst = max(worst, float(np.nanmax(fraction)))
    print(f"coupling, the kernel's form in numpy: {worst:.4f} of the bar")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ symmetries
def test_rigid_motion_leaves_the_gait_unchanged_with_per_frame_frames():
    rng = np.random.default_rng(4)
    X, _, _ = jo.random_fly(rng, 60)
    R, shift = jo.random_rotation(rng), rng.normal(size=3)
    a = go.gait(X, 80.0, "per_frame", on=1.0, off=-1.0)
    b = go.gait(X @ R.T + shift, 80.0, "per_frame", on=1.0, off=-1.0)
    assert np.allclose(a["tip"], b["tip"], atol=1e-12, equal_nan=True)
    # the velocity is taken in frame t's own axes, which turn with the fly: it is the same up to rounding, and so are the states
    # wherever the velocity is not within rounding of a threshold
    assert np.allclose(a["vel"], b["vel"], atol=1e-9, equal_nan=True)
    clear = np.all((np.abs(a["vel"][..., 0] - 1.0) > 1e-6) & (np.abs(a["vel"][..., 0] + 1.0) > 1e-6))
    assert clear and np.array_equal(a["states"], b["states"]) and np.array_equal(a["steps"], b["steps"])
    assert np.array_equal(a["phase"], b["phase"], equal_nan=True) and np.array_equal(a["pattern"], b["pattern"])


def test_mirror_image_with_the_sides_swapped_is_exactly_equal():
    X = go.random_poses(200, seed=5)
    M = X.copy()
    M[:, :19], M[:, 19:] = X[:, 19:], X[:, :19]
    M[..., 1] = -M[..., 1]
    a = go.gait(X, 100.0, np.eye(3), on=2.0, off=-2.0)
    b = go.gait(M, 100.0, np.eye(3), on=2.0, off=-2.0)
    swap = [3, 4, 5, 0, 1, 2]
    assert a["tip"][:, swap].tobytes() == b["tip"].tobytes() and a["vel"][:, swap].tobytes() == b["vel"].tobytes()
    assert np.array_equal(a["states"][:, swap], b["states"]) and a["phase"][:, swap].tobytes() == b["phase"].tobytes()
    assert np.array_equal(a["state_counts"][swap], b["state_counts"])
    assert np.array_equal(a["coupling_count"][np.ix_(swap, swap)], b["coupling_count"])


# ------------------------------------------------------------------------------------------------------------------ the planted walker
def test_planted_walker_recovered_by_the_oracle_alone(golden_dir):
    X = go.planted_walker(go.planted_pose(golden_dir))
    assert X.shape == (go.PLANTED["T"], 38, 3)
    r = go.gait(X, go.PLANTED["fps"])   # the default thresholds, the recording frame
    go.check_planted(r)
    swing, stance = r["step_metrics"][:, 0], r["step_metrics"][:, 1]
    assert np.all(np.abs(swing + stance - 0.2) < 1e-12) and np.all(np.abs(swing - 0.09) < 1e-12)   # 9 of 20 frames: the window's half frame at both ends
    assert np.all(np.abs(r["step_metrics"][:, 2] - r["step_metrics"][0, 2]) < 1e-9) and r["step_metrics"][0, 2] > 2.5


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_config_names():
    from deepfly3d_amd import config as cfg

    assert (cfg.GAIT_DIFF_HALF, cfg.GAIT_SWING_ON, cfg.GAIT_SWING_OFF) == (go.HALF, go.ON, go.OFF)
    assert cfg.GAIT_DIFF_HALF_RANGE == (1, 64) and cfg.GAIT_TRIPODS == go.TRIPODS == (21, 42)
    assert [sum(1 << leg for leg in legs) for legs in ((0, 2, 4), (1, 3, 5))] == list(cfg.GAIT_TRIPODS)


def test_ops_refusals():
    from deepfly3d_amd import ops

    assert ops.gait_thresholds() == (go.ON, go.OFF, go.HALF) and ops.gait_thresholds(3, -1.5, 7) == (3.0, -1.5, 7)
    for on, off in ((NAN, 0.0), (5.0, NAN), (np.inf, 0.0), (5.0, -np.inf)):
        with pytest.raises(ValueError, match="on and off must be finite"):
            ops.gait_thresholds(on, off)
    for on, off in ((0.0, 0.0), (1.0, 2.0), (None, 5.0), (0.0, None), (-1.0, None)):
        with pytest.raises(ValueError, match="on must be above off"):
            ops.gait_thresholds(on, off)
    for w in (0, 65, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match=r"half_window must be an integer in \[1, 64\]"):
            ops.gait_thresholds(half_window=w)
    host = torch.zeros((4, 38, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"points3d must be a torch.float64 CUDA tensor of shape \[T, 38, 3\]"):
        ops.tip_kinematics(host, 100.0)
    with pytest.raises(ValueError, match="points3d must be"):
        ops.gait(np.zeros((4, 38, 3)), 100.0)
    for fps in (0.0, -1.0, NAN, np.inf, None, "100", True):
        with pytest.raises(ValueError, match="fps must be a finite number > 0"):
            ops.gait(host, fps)
    with pytest.raises(ValueError, match="on must be above off"):
        ops.gait(host, 100.0, on=0.0)
    with pytest.raises(ValueError, match="half_window must be"):
        ops.gait(host, 100.0, half_window=0)
    with pytest.raises(ValueError, match=r"vel must be a torch.float64 CUDA tensor of shape \[T, 6, 3\]"):
        ops.gait_states(torch.zeros((4, 6, 3), dtype=torch.float64))
    states = torch.zeros((4, 6), dtype=torch.int32)
    for call in (lambda: ops.gait_steps(states, torch.zeros((4, 6, 3), dtype=torch.float64), 100.0), lambda: ops.gait_phase(states),
                 lambda: ops.gait_patterns(states)):
        with pytest.raises(ValueError, match=r"states must be a torch.int32 CUDA tensor of shape \[T, 6\]"):
            call()
    with pytest.raises(ValueError, match=r"phase must be a torch.float64 CUDA tensor of shape \[T, 6\]"):
        ops.gait_coupling(torch.zeros((4, 6), dtype=torch.float64))
    import dataclasses

    assert [f.name for f in dataclasses.fields(ops.GaitResult)] == ["tip", "vel", "states", "steps", "step_metrics", "phase", "coupling",
                                                                    "coupling_count", "pattern", "pattern_histogram", "state_counts",
                                                                    "thresholds", "fps"]


def test_pose_chain_needs_fps():
    from deepfly3d_amd.kinematics import PoseChain

    with pytest.raises(ValueError, match="without the recording's fps"):
        PoseChain(torch.zeros((4, 38, 3), dtype=torch.float64)).gait()


def test_command_line_refusals(capsys):
    from deepfly3d_amd import cli

    for argv, message in ((["x", "--gait-on", "3"], "--gait-on sets the swing threshold of --gait: it needs --gait"),
                          (["x", "--gait-off", "-1"], "--gait-off sets the stance threshold of --gait: it needs --gait"),
                          (["x", "--gait", "--gait-on", "0"], "on must be above off"),
                          (["x", "--gait", "--gait-off", "5"], "on must be above off"),
                          (["x", "--gait", "--gait-on", "nan"], "on and off must be finite"),
                          (["x", "--gait", "--gait-off=-inf"], "on and off must be finite")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err)
    args = cli.parse_cli_args(["x", "--gait", "--gait-on", "7.5", "--gait-off", "-2", "--rigid-legs", "--skip-pose-estimation"])
    assert args.gait and args.gait_on == 7.5 and args.gait_off == -2.0 and args.rigid_legs and args.skip_estimation
    args = cli.parse_cli_args(["x"])
    assert not args.gait and args.gait_on is None and args.gait_off is None


def _one_frame_folder(tmp_path, golden_dir):
    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    return str(folder)


def test_cli_gait_without_a_result_to_reopen_is_refused(tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    args = cli.parse_cli_args([folder, "--gait", "--skip-pose-estimation"])
    with pytest.raises(RuntimeError, match="--gait needs calibrated cameras"):
        cli.run(args)
    config.pop("image_shape", None)
    assert not [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]


def test_core_refusals(tmp_path, golden_dir):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    with pytest.raises(RuntimeError, match="gait needs calibrated cameras"):
        core.gait()
    with pytest.raises(ValueError, match="on must be above off"):   # before the cameras are asked for
        core.gait(on=-1.0)
    with pytest.raises(ValueError, match="half_window must be"):
        core.gait(half_window=100)
    with pytest.raises(ValueError, match="fps must be a finite number > 0"):
        core.gait(fps=0.0)
    with pytest.raises(ValueError, match="gait_on and gait_off belong to gait: they need gait=True"):
        core.save(gait_on=3.0)
    with pytest.raises(ValueError, match="on must be above off"):
        core.save(gait=True, gait_off=9.0)
    config.pop("image_shape", None)
