"""CPU tests of the pose repair's model (tests/pose_repair_oracle.py) on hand-written rows, of the planted walker
with noise and spikes, proved by the oracle alone, and of every refusal of ops, Core and the command line, which come before any
device work."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402
import joint_angles_oracle as jo  # noqa: E402
import pose_repair_oracle as pr  # noqa: E402

NAN, INF = float("nan"), float("inf")
SCALE = pr.K * pr.MAD_TO_SIGMA


def _pose(series, joint=0, coordinate=0, T=None):
    """[T, 38, 3]: every joint at (1, 2, 3) in every frame, `series` in one coordinate of one joint."""
    series = np.asarray(series, dtype=np.float64)
    X = np.tile(np.array([1.0, 2.0, 3.0]), (len(series) if T is None else T, 38, 1))
    X[:len(series), joint, coordinate] = series
    return X


def _outlier(flags):
    return (flags & 2).astype(bool)


# ------------------------------------------------------------------------------------------------------------------ the Hampel test
def test_constant_series_and_the_floor():
    X = _pose(np.full(20, 4.0))
    X[7, 0, 0] += 0.06   # mad = 0: thr = floor
    flags, score = pr.outliers(X)
    assert _outlier(flags).sum() == 1 and flags[7, 0] == 2
    assert score[7, 0] == np.float64(4.0 + 0.06 - 4.0) / 0.05 and np.all(score[np.arange(20) != 7] == 0.0)
    X[7, 0, 0] = 4.0 + 0.04
    assert not pr.outliers(X)[0].any()
    # floor = 0: a constant series flags nothing (dev = 0 is never > 0) and scores 0; any deviation from it scores +inf
    flags, score = pr.outliers(_pose(np.full(20, 4.0)), floor=0.0)
    assert not flags.any() and np.all(score == 0.0)
    flags, score = pr.outliers(X, floor=0.0)
    assert flags[7, 0] == 2 and score[7, 0] == INF and _outlier(flags).sum() == 1


def test_a_deviation_equal_to_the_bound_is_kept():
    X = _pose(np.zeros(7))
    X[3, 0, 0] = 0.5   # mad = 0, so thr = floor
    flags, score = pr.outliers(X, h=2, floor=0.5)
    assert not flags.any() and score[3, 0] == 1.0          # dev == thr: kept, by plain >
    flags, score = pr.outliers(X, h=2, floor=np.nextafter(0.5, 0.0))
    assert flags[3, 0] == 2 and score[3, 0] > 1.0
    # the same with a bound from the mad.  Frame 2 at h = 2 sees all five: m = 3, dev = (3, 2, 7, 0, 1), mad = 2
    X = _pose(np.array([0.0, 1.0, 10.0, 3.0, 4.0]))
    flags, score = pr.outliers(X, h=2, k=1.0, floor=0.0)
    assert score[2, 0] == 7.0 / (1.0 * 1.4826 * 2.0) and flags[2, 0] == 2
    flags, score = pr.outliers(X, h=2, k=3.5 / 1.4826 * 1.0000001, floor=0.0)   # thr just above 7
    assert flags[2, 0] == 0 and 0.999999 < score[2, 0] < 1.0
    flags, score = pr.outliers(X, h=2, k=2.0, floor=7.0)   # scale * mad = 5.9304 < floor = 7 = dev
    assert flags[2, 0] == 0 and score[2, 0] == 1.0


def test_even_and_odd_counts_and_the_clipped_window():
    series = np.array([5.0, 1.0, 4.0, 2.0, 3.0, 9.0])
    X = _pose(series)
    _, score = pr.outliers(X, h=2, k=1.0, floor=0.0, n_min=1)
    loop = pr.outliers_loop(X, h=2, k=1.0, floor=0.0, n_min=1)[1]
    assert np.array_equal(score, loop)
    # frame 0: the window is clipped to frames 0 .. 2 = (5, 1, 4): odd, m = 4, dev (1, 3, 0), mad = 1
    assert score[0, 0] == 1.0 / (1.4826 * 1.0)
    # frame 1: frames 0 .. 3 = (5, 1, 4, 2): even, m = (2 + 4) / 2 = 3, dev (2, 2, 1, 1), mad = (1 + 2) / 2
    assert score[1, 0] == 2.0 / (1.4826 * 1.5)
    # frame 5: clipped at the other end, frames 3 .. 5 = (2, 3, 9): m = 3, dev (1, 0, 6), mad = 1
    assert score[5, 0] == 6.0 / (1.4826 * 1.0)
    # T < 2 h + 1: clipped at both ends in every frame
    X = _pose(np.array([1.0, 2.0, 40.0]))
    flags, score = pr.outliers(X, h=64, k=1.0, floor=0.0)
    assert flags[:, 0].tolist() == [0, 0, 2] and score[2, 0] == 38.0 / 1.4826 and score[1, 0] == 0.0
    assert np.array_equal(score, pr.outliers_loop(X, h=64, k=1.0, floor=0.0)[1])


def test_too_few_valid_frames_are_untested():
    X = _pose(np.array([1.0, 50.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]))
    X[[0, 2, 3], 0] = 0.0   # frame 1's window (h = 2) holds frame 1 alone
    flags, score = pr.outliers(X, h=2, n_min=2)
    assert flags[:4, 0].tolist() == [1, 0, 1, 1] and np.isnan(score[:4, 0]).all()   # n = 1 = n_min - 1: untested, not an outlier
    flags, score = pr.outliers(X, h=2, n_min=1)
    assert flags[1, 0] == 0 and score[1, 0] == 0.0    # tested against itself
    X[3, 0] = [1.0, 2.0, 3.0]   # n = 2 = n_min: m = 25.5, dev (24.5, 24.5), mad = 24.5: kept
    flags, score = pr.outliers(X, h=2, n_min=2)
    assert flags[1, 0] == 0 and score[1, 0] == 24.5 / (SCALE * 24.5)
    for T in (1, 2):   # with the default n_min = 3 a recording of one or two frames is untested throughout
        flags, score = pr.outliers(_pose(np.arange(T, dtype=np.float64) + 1.0))
        assert not flags.any() and np.isnan(score).all()
    flags, score = pr.outliers(_pose(np.array([7.0])), n_min=1)
    assert not flags.any() and np.all(score == 0.0)
    assert pr.outliers(np.zeros((0, 38, 3)))[0].shape == (0, 38)


def test_missing_joints():
    X = _pose(np.arange(12, dtype=np.float64) * 0.001)
    X[2, 5] = [NAN, 2.0, 3.0]
    X[3, 5] = [1.0, INF, 3.0]
    X[4, 5] = 0.0
    X[5, 5] = [-0.0, 0.0, 0.0]
    X[6, 5] = [0.0, 0.0, 1e-300]   # not missing
    flags, score = pr.outliers(X, floor=1e6)
    assert flags[:, 5].tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0] and np.isnan(score[2:6, 5]).all() and np.isfinite(score[6, 5])
    assert (flags == 1).sum() == 4
    # the missing frames take no part in the windows of their neighbours: frame 6 at h = 1 sees itself and frame 7 alone, whatever the
    # non-finite numbers before it
    pair = _pose(np.array([1.0, 1.0]))
    pair[:, 5] = X[6:8, 5]
    assert pr.outliers(X, h=1, n_min=1)[1][6, 5] == pr.outliers(pair, h=1, n_min=1)[1][0, 5] > 0.0
    Y, status, counts = pr.fill_gaps(X, flags)
    assert status[2:6, 5].tolist() == [1, 1, 1, 1] and np.isfinite(Y).all() and counts[5].tolist() == [8, 4, 0, 0, 0]


def test_a_spike_in_one_coordinate_only():
    rng = np.random.default_rng(0)
    X = rng.normal(0.0, 0.01, (50, 38, 3)) + 1.0
    X[20, 9, 1] += 2.0
    flags, score = pr.outliers(X)
    assert _outlier(flags).sum() == 1 and flags[20, 9] == 2 and score[20, 9] > 10.0
    assert np.array_equal(flags, pr.outliers_loop(X)[0]) and np.array_equal(score, pr.outliers_loop(X)[1])
    # the score is the largest of the three coordinates'
    alone = X.copy()
    alone[:, 9, [0, 2]] = 1.0   # the other two coordinates constant: their score is 0
    assert pr.outliers(alone)[1][20, 9] == score[20, 9]


def test_the_medians_are_numpys():
    rng = np.random.default_rng(1)
    for n in range(1, 14):
        v = rng.normal(size=n)
        v[rng.integers(0, n, 2)] = v[0]   # ties
        assert pr.median_sorted(np.sort(v)) == np.median(v)
    # and the vectorised windows', on the same valid sets
    T, h = 40, 3
    X = pr.tied_poses(T, h, seed=2)
    miss = pr.missing(X)
    padded_valid = np.zeros((T + 2 * h, 38), dtype=bool)
    padded_valid[h:h + T] = ~miss
    padded = np.zeros((T + 2 * h, 38))
    padded[h:h + T] = np.where(miss, 0.0, X[..., 1])
    from numpy.lib.stride_tricks import sliding_window_view as view

    vw, xw = view(padded_valid, 2 * h + 1, axis=0), view(padded, 2 * h + 1, axis=0)
    got = pr._window_median(xw, vw, vw.sum(-1))
    for t in range(T):
        for j in range(38):
            if vw[t, j].any():
                assert got[t, j] == np.median(xw[t, j][vw[t, j]]), (t, j)


def test_the_vectorised_oracle_is_the_loop():
    for T, h, n_min in ((1, 1, 1), (2, 2, 2), (7, 5, 3), (61, 1, 3), (61, 2, 5), (300, 5, 3), (140, 64, 129)):
        X = pr.tied_poses(T, h, seed=T + h)
        a, b = pr.outliers(X, h, n_min=n_min), pr.outliers_loop(X, h, n_min=n_min)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True), (T, h)
        for gap in (0, 1, 7, 1000000):
            f, g = pr.fill_gaps(X, a[0], gap), pr.fill_gaps_loop(X, a[0], gap)
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(f, g)), (T, h, gap)


# ------------------------------------------------------------------------------------------------------------------ gaps
def _gap_case(T, bad):
    X = _pose(np.arange(T, dtype=np.float64) * 0.25 + 1.0, joint=4, coordinate=2)
    flags = np.zeros((T, 38), dtype=np.uint8)
    flags[list(bad), 4] = 1
    X[list(bad), 4] = 0.0
    return X, flags


def test_gap_lengths():
    X, flags = _gap_case(30, range(5, 15))   # ten frames
    for gap, code in ((10, pr.MISSING_FILLED), (9, pr.MISSING_LEFT), (0, pr.MISSING_LEFT)):
        Y, status, counts = pr.fill_gaps(X, flags, gap)
        assert np.all(status[5:15, 4] == code) and (status != 0).sum() == 10 and counts[4].tolist()[code] == 10 and counts[4, 0] == 20
        if code == pr.MISSING_FILLED:
            assert np.all(np.abs(Y[5:15, 4, 2] - (np.arange(5, 15) * 0.25 + 1.0)) <= 2.0 ** -52 * 4.0) and np.all(Y[5:15, 4, :2] == [1.0, 2.0])
        else:
            assert not Y[5:15, 4].any() and not np.signbit(Y[5:15, 4]).any()   # +0.0: missing
    X, flags = _gap_case(30, range(5, 16))   # max_gap + 1 frames: left
    assert np.all(pr.fill_gaps(X, flags, 10)[1][5:16, 4] == pr.MISSING_LEFT)
    X, flags = _gap_case(30, [7])
    flags[7, 4] = 2   # an outlier
    assert pr.fill_gaps(X, flags, 0)[1][7, 4] == pr.OUTLIER_REMOVED and pr.fill_gaps(X, flags, 1)[1][7, 4] == pr.OUTLIER_FILLED
    flags[7, 4] = 3   # both bits: bit 0 decides
    assert pr.fill_gaps(X, flags, 1)[1][7, 4] == pr.MISSING_FILLED


def test_gaps_at_the_ends_and_a_joint_missing_throughout():
    X, flags = _gap_case(20, [0, 1, 18, 19, 9])
    flags[9, 4] = 2
    Y, status, counts = pr.fill_gaps(X, flags, 1000000)   # no extrapolation, however long a gap may be
    assert status[:, 4].tolist() == [3, 3] + [0] * 7 + [2] + [0] * 8 + [3, 3] and not Y[[0, 1, 18, 19], 4].any()
    assert counts[4].tolist() == [15, 0, 1, 4, 0] and np.all(counts.sum(axis=1) == 20)
    X, flags = _gap_case(20, range(20))
    Y, status, counts = pr.fill_gaps(X, flags)
    assert np.all(status[:, 4] == pr.MISSING_LEFT) and not Y[:, 4].any() and counts[4].tolist() == [0, 0, 0, 20, 0]
    assert np.array_equal(Y[:, :4], X[:, :4]) and np.all(status[:, :4] == 0)
    # T = 1
    X, flags = _gap_case(1, [0])
    Y, status, counts = pr.fill_gaps(X, flags)
    assert status[0, 4] == pr.MISSING_LEFT and counts.sum() == 38 and counts[4, 3] == 1
    r = pr.repair(np.zeros((0, 38, 3)))
    assert r["points"].shape == (0, 38, 3) and r["status"].shape == (0, 38) and not r["counts"].any() and r["counts"].shape == (38, 5)


def test_interpolation_of_an_affine_series_is_exact_to_one_rounding():
    rng = np.random.default_rng(3)
    T = 200
    slope, start = rng.normal(size=(38, 3)), rng.normal(size=(38, 3))
    X = start + slope * np.arange(T)[:, None, None]
    flags = (rng.random((T, 38)) < 0.3).astype(np.uint8)
    flags[[0, -1]] = 0
    Y, status, counts = pr.fill_gaps(X, flags, T)
    assert np.all((status == pr.MISSING_FILLED) == (flags == 1)) and np.all(counts.sum(axis=1) == T)
    # the value passes through a subtraction, a division, a product and a sum: each within one rounding of magnitudes <= |A| + |B|
    bound = 4.0 * 2.0 ** -53 * (np.abs(start) + np.abs(slope) * T) * 2.0
    assert np.all(np.abs(Y - X) <= bound) and np.array_equal(Y[flags == 0], X[flags == 0])
    # a gap whose ends are equal is filled with that value exactly; half-way between two values is their mean to one rounding
    X = _pose(np.array([2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 5.0]), joint=1)
    flags = np.zeros((7, 38), dtype=np.uint8)
    flags[[1, 2, 3, 5], 1] = 2
    Y = pr.fill_gaps(X, flags)[0]
    assert Y[:, 1, 0].tolist() == [2.0, 2.0, 2.0, 2.0, 2.0, 3.5, 5.0]


def test_good_joints_keep_their_bits():
    X = pr.tied_poses(300, 5, seed=9)
    r = pr.repair(X)
    kept = r["status"] == 0
    assert X[kept].tobytes() == r["points"][kept].tobytes() and np.all(r["counts"].sum(axis=1) == 300)
    assert np.all((r["status"] == 0) == (r["flags"] == 0)) and not pr.missing(r["points"])[(r["status"] == 1) | (r["status"] == 2)].any()
    assert pr.missing(r["points"])[r["status"] >= 3].all() and np.all(r["status"][:, 11] == pr.MISSING_LEFT)


# ------------------------------------------------------------------------------------------------------------------ the planted walker
# the smallest score of a spike, per half window, as the oracle gives it for this file's generator (planted_spikes, seed 1): a spike is
# flagged when its score exceeds 1, and the +-8 mm on a tip that sweeps 3.2 mm comes closer to 1 the more of the sweep the window holds
SPIKE_SCORE = {2: 1.47, 3: 1.47, 5: 1.29, 8: 1.07}


@pytest.mark.parametrize("h", sorted(SPIKE_SCORE))
def test_planted_spikes_found_by_the_oracle_alone(golden_dir, h):
    pose = go.planted_pose(golden_dir)
    X, placed = pr.planted_spikes(pr.noisy_walker(pose), h)
    assert len(placed) == 60 and pr.missing(X).sum() == 2
    r = pr.repair(X, h=h)
    spikes = np.zeros((len(X), 38), dtype=bool)
    spikes[tuple(np.array(placed).T)] = True
    assert np.array_equal(_outlier(r["flags"]), spikes)   # all planted, no others
    print(f"h = {h}: clean max {np.nanmax(r['score'][~spikes]):.4f}, spike min {r['score'][spikes].min():.4f}")
    assert np.nanmax(r["score"][~spikes]) <= 0.47 and r["score"][spikes].min() >= SPIKE_SCORE[h]
    assert r["counts"].sum(axis=0).tolist() == [len(X) * 38 - 62, 2, 60, 0, 0]
    before, after = go.gait(X, go.PLANTED["fps"]), go.gait(r["points"], go.PLANTED["fps"])
    planted = go.planted_lift_offs()
    want = [(leg, t0, t2) for leg in range(6) for t0, t2 in zip(planted[leg][:-1], planted[leg][1:])]
    assert len(want) == 171 and [(leg, t0, t2) for leg, t0, _, t2 in after["steps"].tolist()] == want   # all 171: the step across the gap is back
    assert [(leg, t0, t2) for leg, t0, _, t2 in before["steps"].tolist()] != want   # the spikes split steps and the gap drops one


def test_the_noiseless_walker(golden_dir):
    pose = go.planted_pose(golden_dir)
    X = go.planted_walker(pose)
    r = pr.repair(X)
    assert not _outlier(r["flags"]).any() and r["counts"].sum(axis=0).tolist() == [len(X) * 38 - 2, 2, 0, 0, 0]
    leg, frames = go.PLANTED["missing_leg"], np.array(go.PLANTED["missing_frames"])
    ex = jo.body_frame(pose)[0]
    planted = pose[go.TIPS[leg]] + go.planted_sawtooth(frames - go.planted_offsets()[leg])[:, None] * ex   # the frames lie in a stance
    assert np.abs(r["points"][frames, go.TIPS[leg]] - planted).max() <= 4.5e-16
    assert len(go.gait(r["points"], go.PLANTED["fps"])["steps"]) == 171 == len(go.gait(X, go.PLANTED["fps"])["steps"]) + 1


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_config_names():
    from deepfly3d_amd import config as cfg

    assert (cfg.REPAIR_HALF_WINDOW, cfg.REPAIR_THRESHOLD, cfg.REPAIR_FLOOR, cfg.REPAIR_MIN_COUNT, cfg.REPAIR_MAX_GAP) == (pr.HALF, pr.K, pr.FLOOR, pr.N_MIN,
                                                                                                                        pr.MAX_GAP)
    assert (pr.HALF, pr.K, pr.FLOOR, pr.N_MIN, pr.MAX_GAP) == (5, 6.0, 0.05, 3, 10)
    assert cfg.REPAIR_HALF_WINDOW_RANGE == (1, 64) and cfg.REPAIR_MAX_GAP_RANGE == (0, 1000000) and cfg.REPAIR_MAD_TO_SIGMA == pr.MAD_TO_SIGMA == 1.4826


def test_ops_refusals():
    from deepfly3d_amd import ops

    assert ops.repair_params() == (5, 6.0, 0.05, 10, 3) and ops.repair_params(2, 3, 0, 0, 5) == (2, 3.0, 0.0, 0, 5)
    assert ops.repair_params(64, 1e-3, 7.5, 1000000, 129) == (64, 1e-3, 7.5, 1000000, 129)
    for h in (0, 65, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match=r"half_window must be an integer in \[1, 64\]"):
            ops.repair_params(half_window=h)
    for k in (0.0, -6.0, NAN, INF):
        with pytest.raises(ValueError, match="threshold must be finite and > 0"):
            ops.repair_params(threshold=k)
    for floor in (-0.05, NAN, INF):
        with pytest.raises(ValueError, match="floor must be finite and >= 0"):
            ops.repair_params(floor=floor)
    for name in ("threshold", "floor"):
        for v in ("6", True, [6.0]):
            with pytest.raises(ValueError, match=f"{name} must be a number"):
                ops.repair_params(**{name: v})
    for gap in (-1, 1000001, 10.0, False, "10"):
        with pytest.raises(ValueError, match=r"max_gap must be an integer in \[0, 1000000\]"):
            ops.repair_params(max_gap=gap)
    for h, n in ((5, 0), (5, 12), (1, 4), (None, 12), (2, 3.0), (2, True)):
        with pytest.raises(ValueError, match=r"min_count must be an integer in \[1, \d+\]"):
            ops.repair_params(half_window=h, min_count=n)
    host = torch.zeros((4, 38, 3), dtype=torch.float64)
    for call in (lambda: ops.pose_outliers(host), lambda: ops.repair_pose(host), lambda: ops.fill_gaps(host, torch.zeros((4, 38), dtype=torch.uint8)),
                 lambda: ops.repair_pose(np.zeros((4, 38, 3))), lambda: ops.pose_outliers(torch.zeros((4, 38, 3)))):
        with pytest.raises(ValueError, match=r"points3d must be a torch.float64 CUDA tensor of shape \[T, 38, 3\]"):
            call()
    with pytest.raises(ValueError, match="threshold must be finite"):   # the parameters come first
        ops.repair_pose(host, threshold=0.0)
    with pytest.raises(ValueError, match="max_gap must be"):
        ops.repair_pose(host, max_gap=-1)
    assert [f.name for f in dataclasses.fields(ops.PoseRepairResult)] == ["points", "status", "counts", "score", "params"]


def test_command_line_refusals(capsys):
    from deepfly3d_amd import cli

    for argv, message in ((["x", "--repair-window", "3"], "--repair-window sets a parameter of --repair-pose: it needs --repair-pose"),
                          (["x", "--repair-threshold", "3"], "--repair-threshold sets a parameter of --repair-pose: it needs --repair-pose"),
                          (["x", "--repair-floor", "0.1"], "--repair-floor sets a parameter of --repair-pose: it needs --repair-pose"),
                          (["x", "--repair-max-gap", "3"], "--repair-max-gap sets a parameter of --repair-pose: it needs --repair-pose"),
                          (["x", "--repair-pose", "--repair-window", "0"], r"half_window must be an integer in \[1, 64\]"),
                          (["x", "--repair-pose", "--repair-window", "65"], r"half_window must be an integer in \[1, 64\]"),
                          (["x", "--repair-pose", "--repair-window", "2.5"], "invalid int value"),
                          (["x", "--repair-pose", "--repair-threshold", "0"], "threshold must be finite and > 0"),
                          (["x", "--repair-pose", "--repair-threshold", "nan"], "threshold must be finite and > 0"),
                          (["x", "--repair-pose", "--repair-floor=-1"], "floor must be finite and >= 0"),
                          (["x", "--repair-pose", "--repair-floor", "inf"], "floor must be finite and >= 0"),
                          (["x", "--repair-pose", "--repair-max-gap=-1"], r"max_gap must be an integer in \[0, 1000000\]"),
                          (["x", "--repair-pose", "--repair-max-gap", "1000001"], r"max_gap must be an integer in \[0, 1000000\]")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err), argv
    args = cli.parse_cli_args(["x", "--repair-pose", "--repair-window", "8", "--repair-threshold", "4.5", "--repair-floor", "0", "--repair-max-gap", "0",
                               "--gait", "--skip-pose-estimation"])
    assert args.repair_pose and (args.repair_window, args.repair_threshold, args.repair_floor, args.repair_max_gap) == (8, 4.5, 0.0, 0) and args.gait
    args = cli.parse_cli_args(["x"])
    assert not args.repair_pose and args.repair_window is None and args.repair_threshold is None and args.repair_floor is None and args.repair_max_gap is None
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for option in ("--repair-window H", "--repair-threshold K", "--repair-floor MM", "--repair-max-gap N"):
        assert option in text
    assert "guesses that nobody has measured on a recording" in text and "blind to a spike smaller than" in text


def _one_frame_folder(tmp_path, golden_dir):
    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    return str(folder)


def test_cli_repair_without_a_result_to_reopen_is_refused(tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    args = cli.parse_cli_args([folder, "--repair-pose", "--skip-pose-estimation"])
    with pytest.raises(RuntimeError, match="--repair-pose needs calibrated cameras"):
        cli.run(args)
    config.pop("image_shape", None)
    assert not [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]


def test_core_refusals(tmp_path, golden_dir):
    import inspect

    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    with pytest.raises(RuntimeError, match="repair_pose needs calibrated cameras"):
        core.repair_pose()
    with pytest.raises(ValueError, match="half_window must be"):   # before the cameras are asked for
        core.repair_pose(half_window=0)
    with pytest.raises(ValueError, match="threshold must be finite"):
        core.repair_pose(threshold=-1.0)
    with pytest.raises(ValueError, match="floor must be finite"):
        core.repair_pose(floor=NAN)
    with pytest.raises(ValueError, match="max_gap must be"):
        core.repair_pose(max_gap=2000000)
    with pytest.raises(ValueError, match="min_count must be"):
        core.repair_pose(half_window=1, min_count=4)
    for name in ("joint_angles", "rigid_legs", "angle_spectrogram", "behaviour_map", "behaviour_segments", "gait"):
        with pytest.raises(RuntimeError, match=f"{name} needs calibrated cameras"):
            getattr(core, name)(repair=True)
        named = [p for p in inspect.signature(getattr(Core, name)).parameters.values() if p.kind != p.VAR_KEYWORD]
        assert named[-1].name == "repair" and named[-1].default is False   # the last keyword
    for option in ("repair_window", "repair_threshold", "repair_floor", "repair_max_gap"):
        with pytest.raises(ValueError, match="belong to repair_pose: they need repair_pose=True"):
            core.save(**{option: 1})
    with pytest.raises(ValueError, match="half_window must be"):
        core.save(repair_pose=True, repair_window=65)
    with pytest.raises(ValueError, match="threshold must be finite"):
        core.save(repair_pose=True, repair_threshold=0.0)
    with pytest.raises(ValueError, match="floor must be finite"):
        core.save(repair_pose=True, repair_floor=-1.0)
    with pytest.raises(ValueError, match="max_gap must be"):
        core.save(repair_pose=True, repair_max_gap=-1)
    config.pop("image_shape", None)
