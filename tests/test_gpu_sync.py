"""-m gpu tests of the camera-lag stage (csrc/sync.hip).  The cost tables, the lag paths and the gather equal
tests/sync_oracle.py exactly: a sample's cost is rounded once to int64 and everything after it is integer arithmetic.  The margins are
the oracle's float64 divisions in the same order (bar 1e-12 relative)."""
import os
import pickle

import numpy as np
import pytest
import torch

import sync_cases as sc
import sync_oracle as so
from deepfly3d_amd import sync

pytestmark = pytest.mark.gpu

FRAME_CHUNK = 4   # the frames a workgroup of pair_costs_kernel takes per step (csrc/sync.hip: FRAMES)
LAG_GROUP = 3     # the lags of a workgroup (csrc/sync.hip: LAGS)


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)


def _all_pairs(C):
    return np.array([(a, b) for a in range(C) for b in range(a + 1, C)], dtype=np.int32)


def _random_case(C, T, J, seed, hidden=0.1):
    """(px [C, T, J, 2] in 1 .. 900 px with a share of unseen detections, pairs: all, F: random 3 x 3 of unit norm)."""
    rng = np.random.default_rng(seed)
    px = rng.uniform(1.0, 900.0, size=(C, T, J, 2))
    px[rng.random((C, T, J)) < hidden] = 0.0
    pairs = _all_pairs(C)
    F = rng.normal(size=(len(pairs), 9))
    F /= np.sqrt((F * F).sum(axis=1, keepdims=True))
    return px, pairs, F


def _check_tables(cuda, px, pairs, F, D, W, tau, what):
    """Device tables against the oracle's, then the paths on them; returns the host tables."""
    cost, count = sync.sync_pair_costs(_dev(px, cuda), F, pairs, D, W, tau)
    want_cost, want_count = so.pair_costs(F, pairs, px, D, W, tau)
    got_cost, got_count = cost.cpu().numpy(), count.cpu().numpy()
    assert got_cost.dtype == np.int64 and got_count.dtype == np.int64 and got_cost.shape == want_cost.shape == (len(pairs), so.windows(px.shape[1], W), 2 * D + 1)
    assert np.array_equal(got_count, want_count), (what, "count", int((got_count != want_count).sum()))
    assert np.array_equal(got_cost, want_cost), (what, "cost", int((got_cost != want_cost).sum()))
    for switch, min_count in ((0.0, 1), (3.0, 2), (1000.0, 10 ** 6)):
        _check_paths(cost, count, switch, min_count, what)
    return got_cost, got_count


def _check_paths(cost, count, switch, min_count, what):
    lag, total, margin = (t.cpu().numpy() for t in sync.sync_paths(cost, count, switch, min_count))
    want = so.paths(cost.cpu().numpy(), count.cpu().numpy(), int(np.floor(switch * 1024 + 0.5)), min_count)
    assert lag.dtype == np.int32 and total.dtype == np.int64 and margin.dtype == np.float64
    assert np.array_equal(lag, want[0]), (what, switch, "lag")
    assert np.array_equal(total, want[1]), (what, switch, "path_cost")
    assert np.array_equal(np.isnan(margin), np.isnan(want[2])), (what, switch, "margin NaN")
    assert np.array_equal(np.isinf(margin), np.isinf(want[2]))
    ok = np.isfinite(want[2])
    assert np.all(np.abs(margin[ok] - want[2][ok]) <= 1e-12 * np.abs(want[2][ok])), (what, switch, "margin")
    return lag, total, margin


@pytest.mark.parametrize("name, C, T, J, D, W", [
    ("windows of 16, 16 and 8", 3, 40, 4, 3, 16),
    ("one window", 3, 40, 4, 3, 64),
    ("windows of one frame", 3, 9, 4, 2, 1),
    ("no lag", 3, 20, 5, 0, 8),
    ("lags beyond the recording", 3, 5, 4, 6, 4),
    ("64 joints, 8 cameras", 8, 6, 64, 2, 4),
    ("one lag group", 2, 24, 3, (LAG_GROUP - 1) // 2, 8),
    ("a lag more than a group", 2, 24, 3, (LAG_GROUP + 1) // 2, 8),
    ("seven lag groups", 2, 24, 3, 9, 8),
    ("129 lags", 2, 70, 2, 64, 32),
    ("a frame fewer than the chunk", 2, FRAME_CHUNK - 1, 3, 1, 16),
    ("the chunk", 2, FRAME_CHUNK, 3, 1, 16),
    ("a frame more than the chunk", 2, FRAME_CHUNK + 1, 3, 1, 16),
    ("two chunks and a frame", 2, 2 * FRAME_CHUNK + 1, 3, 1, 16),
    ("windows of 7 and 6", 2, 13, 38, 2, 7),
])
def test_tables_and_paths_equal_the_oracle(native_lib, cuda, name, C, T, J, D, W):
    px, pairs, F = _random_case(C, T, J, seed=100 + C + T + J + D + W)
    cost, count = _check_tables(cuda, px, pairs, F, D, W, 300.0, name)
    assert count.sum() > 0 and ((cost > 0) & (cost < count * 300 * 300 * 1024)).any()   # some samples below the truncation
    if D >= T:   # every sample of a lag beyond the recording is out of range
        far = np.abs(np.arange(-D, D + 1)) >= T
        assert far.any() and not count[:, :, far].any() and not cost[:, :, far].any() and count[:, :, ~far].any()


def test_tables_of_the_calibrated_rig(native_lib, cuda):
    """The fly layout with real fundamental matrices, every pair asked for: a pair of cameras without a common joint counts nothing."""
    px = sc.planted("jump")[0][:, :40]
    pairs = _all_pairs(7)
    F = sync.fundamental_matrices(sc.cameras(), pairs)
    cost, count = _check_tables(cuda, px, pairs, F, 3, 16, 20.0, "rig")
    shared = sc.visible()
    for k, (a, b) in enumerate(pairs):
        assert bool(count[k].any()) == bool((shared[a] & shared[b]).any()), (a, b)
    assert not count[[k for k, (a, b) in enumerate(pairs) if 3 in (a, b)]].any()   # the front camera sees no joint


def test_unseen_detections_count_nothing(native_lib, cuda):
    """A camera without a detection, and detections with exactly one zero coordinate."""
    px, pairs, F = _random_case(3, 21, 6, seed=7, hidden=0.0)
    px[1] = 0.0
    cost, count = _check_tables(cuda, px, pairs, F, 2, 8, 300.0, "camera 1 empty")
    assert not count[[0, 2]].any() and count[1].all()   # pairs (0, 1) and (1, 2) against (0, 2)
    px, pairs, F = _random_case(2, 21, 6, seed=8, hidden=0.0)
    px[0, 0::3, :, 0] = 0.0    # the row alone
    px[1, 1::3, :, 1] = 0.0    # the column alone
    cost, count = _check_tables(cuda, px, pairs, F, 0, 32, 300.0, "one zero coordinate")
    assert count[0, 0, 0] == 7 * 6   # the frames 2, 5, ... 20


def test_truncation_at_and_beyond_tau(native_lib, cuda):
    """F = [0 0 0; 0 0 -3; 0 4 0]: l = (0, -3, 4 row_a), m = (0, 4, -3 row_b), s = 4 row_a - 3 row_b and the denominator is 25, all exact.
    s = 7, 10 and 22 give e = 1.96, 4 and 19.36 around tau^2 = 4."""
    F = np.array([[0, 0, 0, 0, 0, -3, 0, 4, 0]], dtype=np.float64)
    px = np.zeros((2, 3, 1, 2))
    px[0, :, 0] = [(3.25, 11.0), (4.0, 12.0), (7.0, 13.0)]
    px[1, :, 0] = [(2.0, 5.0), (2.0, 6.0), (2.0, 7.0)]
    pairs = np.array([(0, 1)], dtype=np.int32)
    cost, count = _check_tables(cuda, px, pairs, F, 0, 1, 2.0, "tau")
    assert count[0, :, 0].tolist() == [1, 1, 1]
    assert cost[0, :, 0].tolist() == [int(np.floor(49.0 / 25.0 * 1024 + 0.5)), 4096, 4096]
    zero = sync.sync_pair_costs(_dev(px, cuda), np.zeros((1, 9)), pairs, 0, 1, 2.0)   # F = 0: every denominator is 0, every sample skipped
    assert not zero[0].any().item() and not zero[1].any().item()


def _tables(cuda, rows):
    """(cost, count) [1, nW, nL] device tensors of hand-made costs, 10 samples each."""
    cost = torch.tensor([rows], dtype=torch.int64, device=cuda)
    return cost, torch.full_like(cost, 10)


def test_paths_tie_rules(native_lib, cuda):
    """Ties for the last state and for a predecessor go to the smaller (|d|, d)."""
    flat = _tables(cuda, [[5] * 5] * 4)
    lag, total, margin = _check_paths(*flat, 1.0, 1, "flat")
    assert lag.tolist() == [[0, 0, 0, 0]] and total.tolist() == [20] and margin.tolist() == [[0.0] * 4]
    # -1 and +1 tie in the only window: -1; then -2 and +1 do not tie on |d|: +1
    assert _check_paths(*_tables(cuda, [[9, 3, 9, 3, 9]]), 0.0, 1, "last state")[0].tolist() == [[-1]]
    assert _check_paths(*_tables(cuda, [[3, 9, 9, 3, 9]]), 0.0, 1, "last state")[0].tolist() == [[1]]
    # the last window wants +2 at any price; window 0 is flat, so every predecessor costs the same before the jump is added, and with a
    # free jump every predecessor ties: lag 0
    rows = [[7] * 5, [50, 50, 50, 50, 0]]
    assert _check_paths(*_tables(cuda, rows), 0.0, 1, "predecessor, free")[0].tolist() == [[0, 2]]
    assert _check_paths(*_tables(cuda, rows), 1.0, 1, "predecessor, paid")[0].tolist() == [[2, 2]]
    # predecessors -1 and +1 tie for state 0 when both are cheaper by the jump's price
    rows = [[90, 0, 5, 0, 90], [90, 90, 0, 90, 90]]
    lag, total, _ = _check_paths(*_tables(cuda, rows), 1.0 / 1024, 1, "predecessor -1 / +1")
    assert lag.tolist() == [[-1, 0]] and total.tolist() == [1]
    # a window without evidence between two that lag by +1 inherits the lag; the arg-min of the window alone would be 0
    rows = [[900, 900, 900, 0, 900], [4, 4, 4, 4, 4], [900, 900, 900, 0, 900]]
    assert _check_paths(*_tables(cuda, rows), 64.0, 1, "inherit")[0].tolist() == [[1, 1, 1]]
    # below min_count the margin is NaN; without another lag that has a sample it is +inf
    cost, count = _tables(cuda, [[9, 3, 9]])
    count[0, 0, 0] = count[0, 0, 2] = 0
    assert np.isposinf(_check_paths(cost, count, 0.0, 10, "alone")[2]).all()
    assert np.isnan(_check_paths(cost, count, 0.0, 11, "too few")[2]).all()
    rng = np.random.default_rng(3)
    for nW, D, hi in ((1, 0, 5), (7, 1, 3), (33, 4, 4), (300, 2, 2), (5, 64, 3)):   # small ranges: many ties
        cost = torch.from_numpy(rng.integers(0, hi, size=(3, nW, 2 * D + 1))).to(cuda)
        count = torch.from_numpy(rng.integers(0, 3, size=(3, nW, 2 * D + 1))).to(cuda)
        for switch in (0.0, 1.0 / 1024, 2.0 / 1024):
            _check_paths(cost, count, switch, 1, ("random", nW, D))


def test_apply_sync_is_the_gather(native_lib, cuda):
    rng = np.random.default_rng(4)
    for C, T, J, W in ((3, 10, 4, 4), (8, 9, 64, 1), (2, 7, 5, 16)):
        px = rng.uniform(1.0, 900.0, size=(C, T, J, 2))
        lag = rng.integers(-3, 4, size=(C, so.windows(T, W))).astype(np.int32)
        lag[0, 0], lag[-1, -1] = -2, T   # out of range at both ends
        got = sync.apply_sync(_dev(px, cuda), lag, W).cpu().numpy()
        want = so.apply(px, lag, W)
        assert got.tobytes() == want.tobytes() and not got[0, :min(2, W)].any() and not got[-1, (so.windows(T, W) - 1) * W:].any()
        assert sync.apply_sync(_dev(px, cuda), np.zeros_like(lag), W).cpu().numpy().tobytes() == px.tobytes()


def _fields(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in vars(r).items()}


@pytest.mark.parametrize("name", list(sc.PLANTS))
def test_camera_sync_recovers_the_planted_lags(native_lib, cuda, name):
    from deepfly3d_amd import config as cfg

    px, _, lag = sc.planted(name)
    r = sync.camera_sync(sc.cameras(), _dev(px, cuda), max_lag=sc.MAX_LAG, window=sc.WINDOW)
    assert isinstance(r, sync.SyncResult) and r.params == (sc.MAX_LAG, sc.WINDOW, cfg.SYNC_TAU, cfg.SYNC_SWITCH, cfg.SYNC_MIN_COUNT)
    assert r.lag.dtype == np.int32 and np.array_equal(r.lag, lag), (name, r.lag)
    assert r.status.dtype == np.int8 and np.array_equal(r.status, sc.status_of(name))
    assert r.pairs.tolist() == [[0, 1], [0, 2], [1, 2], [4, 5], [4, 6], [5, 6]] and not r.pair_inconsistency.any()
    # every step against the oracle
    cost, count = so.pair_costs(r.F, r.pairs, px, sc.MAX_LAG, sc.WINDOW, cfg.SYNC_TAU)
    assert np.array_equal(r.pair_cost.cpu().numpy(), cost) and np.array_equal(r.pair_count.cpu().numpy(), count)
    want = so.paths(cost, count, int(np.floor(cfg.SYNC_SWITCH * 1024 + 0.5)), cfg.SYNC_MIN_COUNT)
    assert np.array_equal(r.pair_lag.cpu().numpy(), want[0]) and np.array_equal(r.path_cost.cpu().numpy(), want[1])
    assert np.allclose(r.pair_margin.cpu().numpy(), want[2], rtol=1e-12, atol=0.0) and (want[2] > 1.0).all()
    cams = so.camera_lags(r.pairs, want[0], count, 7)
    assert np.array_equal(r.lag, cams[0]) and np.array_equal(r.status, cams[1]) and np.array_equal(r.pair_inconsistency, cams[2])
    assert r.points2d_px.cpu().numpy().tobytes() == so.apply(px, lag, sc.WINDOW).tobytes()
    # two runs give the same bits in every output
    again = _fields(sync.camera_sync(sc.cameras(), _dev(px, cuda), max_lag=sc.MAX_LAG, window=sc.WINDOW))
    for key, value in _fields(r).items():
        assert value.tobytes() == again[key].tobytes(), key


# ------------------------------------------------------------------------------------------------------------------ Core
def _recording(tmp_path, golden_dir, px, image_shape):
    """(folder, result pickle): T frames (links to the sample's frame 0) and an earlier result that holds `px` and the packaged cameras."""
    import deepfly3d_amd

    folder = tmp_path / "working"
    folder.mkdir()
    for c in range(7):
        for t in range(px.shape[1]):
            os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
    folder = str(folder)
    calib = np.load(os.path.join(os.path.dirname(deepfly3d_amd.__file__), "data", "calib.npz"))
    os.makedirs(folder + "_df3d")
    pkl = os.path.join(folder + "_df3d", "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
    res = {c: {"R": calib["R"][c], "tvec": calib["tvec"][c], "distort": calib["distort"][c], "intr": calib["intr"][c]} for c in range(7)}
    res.update(points2d=px / np.asarray(image_shape[::-1], dtype=np.float64), camera_ordering=np.arange(7),
               heatmap_confidence=np.ones((7, px.shape[1], 19), dtype=np.float32))
    with open(pkl, "wb") as f:
        pickle.dump(res, f)
    return folder, pkl


def _load(pkl):
    with open(pkl, "rb") as f:
        return pickle.load(f)


def _same_value(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same_value(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _mean_error(ops, P, px, cuda):
    err = ops.reprojection_errors(P, _dev(px, cuda))[0]
    return float(err[err > 0].mean())


def test_core_checks_and_undoes_the_jump(native_lib, cuda, tmp_path, golden_dir, caplog):
    from PIL import Image

    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    px, clean, lag = sc.planted("jump")
    shape = Image.open(os.path.join(golden_dir, "images", "camera_0_img_0.jpg")).size   # (width, height)
    folder, pkl = _recording(tmp_path, golden_dir, px, shape)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    core.save()
    plain = _load(pkl)
    assert not any("sync" in str(k) for k in plain)
    params = dict(sync_max_lag=sc.MAX_LAG, sync_window=sc.WINDOW)
    with caplog.at_level("WARNING", logger="df3d.logger"):
        core.save(check_sync=True, **params)
    assert [m for m in caplog.messages if "lags" in m] == [f"camera 5 lags by -1 frames from frame {sc.JUMP_AT} on"]
    run = _load(pkl)
    assert list(run) == list(plain) + list(Core._SYNC_KEYS) and len(Core._SYNC_KEYS) == 9
    assert all(_same_value(run[k], plain[k]) for k in plain)
    assert np.array_equal(run["sync_lag"], lag) and run["sync_status"].tolist() == sc.status_of("jump").tolist()
    nW, nL = sc.T // sc.WINDOW, 2 * sc.MAX_LAG + 1
    assert run["sync_pairs"].shape == (6, 2) and run["sync_pair_lag"].shape == (6, nW) and run["sync_pair_margin"].shape == (6, nW)
    assert run["sync_pair_cost"].shape == (6, nW, nL) and run["sync_pair_cost"].dtype == np.float64 and run["sync_pair_count"].dtype == np.int64
    assert not run["sync_pair_inconsistency"].any()
    assert run["sync_params"].tolist() == [sc.MAX_LAG, sc.WINDOW, cfg.SYNC_TAU, cfg.SYNC_SWITCH, cfg.SYNC_MIN_COUNT]
    r = core.camera_sync(max_lag=sc.MAX_LAG, window=sc.WINDOW)
    assert isinstance(r, sync.SyncResult) and all(isinstance(v, (np.ndarray, tuple)) for v in vars(r).values())
    assert _same_value(r.lag, run["sync_lag"]) and _same_value(r.pair_count, run["sync_pair_count"]) and _same_value(r.pair_margin, run["sync_pair_margin"])
    with np.errstate(all="ignore"):
        assert _same_value(run["sync_pair_cost"], r.pair_cost / r.pair_count.astype(np.float64) / 1024.0)
    # undone: every stage of the save sees the shifted detections, the object keeps its own
    own = core.camNet.points2d.copy()
    core.save(sync_cameras=True, joint_angles=True, **params)
    run = _load(pkl)
    assert list(run) == list(plain) + ["joint_angles", "segment_lengths"] + list(Core._SYNC_KEYS) + ["points2d_unsynced"]
    assert _same_value(run["points2d_unsynced"], plain["points2d"]) and _same_value(core.camNet.points2d, own)
    scale = np.asarray(core.image_shape[::-1], dtype=np.float64)
    assert _same_value(run["points2d"], so.apply(plain["points2d"], lag, sc.WINDOW))
    P = np.stack([c.P for c in core.camNet.cam_list])
    shifted = so.apply(own, lag, sc.WINDOW)
    assert _same_value(run["points3d_wo_procrustes"], ops.triangulate(P, _dev(shifted, cuda)).cpu().numpy())
    assert np.array_equal(run["joint_angles"], ops.joint_angles(_dev(run["points3d_wo_procrustes"], cuda))[0].cpu().numpy(), equal_nan=True)
    assert _same_value(core.camNet.points3d, plain["points3d_wo_procrustes"])   # as a plain save leaves it
    synced, unsynced, base = (_mean_error(ops, P, a, cuda) for a in (run["points2d"] * scale, own, clean))
    print(f"mean reprojection error: clean {base:.4f} px, lagging {unsynced:.4f} px, after sync_cameras {synced:.4f} px")
    assert unsynced > synced and abs(synced - base) <= 0.05 * base
    with pytest.raises(ValueError, match="cannot follow auto_correct"):
        core.save(sync_cameras=True, heatmap_triangulation=True)
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_sync_cameras(native_lib, cuda, tmp_path, golden_dir):
    from PIL import Image

    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    px, _, lag = sc.planted("late")
    shape = Image.open(os.path.join(golden_dir, "images", "camera_0_img_0.jpg")).size
    folder, pkl = _recording(tmp_path, golden_dir, px[:, :48], shape)
    order = [str(c) for c in range(7)]
    argv = [folder, "--skip-pose-estimation", "--sync-cameras", "--sync-max-lag", "3", "--sync-window", "16", "--sync-tau", "15", "--sync-switch", "32"]
    assert cli.main(argv + ["--order"] + order) == 0
    run = _load(pkl)
    assert list(run)[-10:] == list(Core._SYNC_KEYS) + ["points2d_unsynced"]
    assert run["sync_params"].tolist()[:4] == [3.0, 16.0, 15.0, 32.0] and np.array_equal(run["sync_lag"], lag[:, :3])
    assert not run["points2d"][1, -2:].any() and run["points2d_unsynced"][1, -2:].any()   # camera 1 has no frames 48 and 49
    config.pop("image_shape", None)
