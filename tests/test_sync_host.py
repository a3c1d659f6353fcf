"""Host tests of the camera-lag stage: the fundamental matrices, the model itself on planted recordings
(tests/sync_oracle.py alone), the cameras' lags from hand-made tables, and every refusal.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import sync_cases as sc
import sync_oracle as so
from deepfly3d_amd import sync

NAN = float("nan")


def _all_pairs(C):
    return np.array([(a, b) for a in range(C) for b in range(a + 1, C)], dtype=np.int32)


def test_fundamental_matrices_annihilate_corresponding_points():
    """|x_b^T F x_a| at rounding level for every pair of the packaged cameras.  F has unit norm, so the nine products and eight sums of
    the form carry at most 11 eps |x_a| |x_b| of rounding; the determinants' LU adds a few eps of relative error to each entry.  The bar
    is 1e-14 |x_a| |x_b| (45 eps, about 5e-9 at these 700 px).  The transposed matrix misses by more than 0.1."""
    P, pairs = sc.cameras(), _all_pairs(7)
    F = sync.fundamental_matrices(P, pairs)
    assert F.shape == (21, 9) and F.dtype == np.float64 and np.allclose((F * F).sum(axis=1), 1.0, rtol=1e-14)
    rng = np.random.default_rng(0)
    x = sc.project(P, sc.FOCUS + rng.uniform(-1.0, 1.0, size=(200, 1, 3)))[:, :, 0]   # [7, 200, (row, col)]
    h = np.stack([x[..., 1], x[..., 0], np.ones(x.shape[:2])], axis=-1)               # (col, row, 1)
    worst = wrong = 0.0
    for k, (a, b) in enumerate(pairs):
        bar = 1e-14 * np.linalg.norm(h[a], axis=1) * np.linalg.norm(h[b], axis=1)
        r = np.abs(np.einsum("ni,ij,nj->n", h[b], F[k].reshape(3, 3), h[a]))
        assert (r <= bar).all(), (a, b, r.max())
        worst = max(worst, float((r / bar).max()))
        wrong = max(wrong, float(np.abs(np.einsum("ni,ij,nj->n", h[a], F[k].reshape(3, 3), h[b])).max()))
    print(f"worst |x_b F x_a| / bar {worst:.2g}; with a and b exchanged up to {wrong:.2g}")
    assert wrong > 0.1
    assert np.array_equal(sync.fundamental_matrices(P, [(2, 5)])[0], F[[tuple(p) for p in pairs].index((2, 5))])
    with pytest.raises(ValueError, match="no fundamental matrix"):
        sync.fundamental_matrices(np.stack([P[0], P[0]]), [(0, 1)])
    for bad in ([(1, 0)], [(0, 7)], [(0, 1), (0, 1)], [(0.0, 1.0)], [0, 1]):
        with pytest.raises(ValueError, match="pairs must"):
            sync.fundamental_matrices(P, bad)
    with pytest.raises(ValueError, match=r"P must be \[ncam, 3, 4\]"):
        sync.fundamental_matrices(P[:, :, :3], pairs)


@pytest.mark.parametrize("name", list(sc.PLANTS))
def test_oracle_recovers_the_planted_lags(name):
    """The model, on the oracle alone: the planted lag in every window, every triangle closed, and the margins DESIGN.md records."""
    from deepfly3d_amd import config as cfg

    px, _, lag = sc.planted(name)
    pairs = so.find_pairs(px, cfg.SYNC_MIN_COUNT)
    assert pairs == [(0, 1), (0, 2), (1, 2), (4, 5), (4, 6), (5, 6)]
    assert sync.sync_pairs(px, cfg.SYNC_MIN_COUNT).tolist() == [list(p) for p in pairs]
    F = sync.fundamental_matrices(sc.cameras(), pairs)
    cost, count = so.pair_costs(F, pairs, px, sc.MAX_LAG, sc.WINDOW, cfg.SYNC_TAU)
    pair_lag, total, margin = so.paths(cost, count, int(np.floor(cfg.SYNC_SWITCH * 1024 + 0.5)), cfg.SYNC_MIN_COUNT)
    got, status, inc = so.camera_lags(pairs, pair_lag, count, 7)
    assert np.array_equal(got, lag), (name, got)
    assert np.array_equal(status, sc.status_of(name)) and not inc.any()
    print(f"{name}: margins {np.nanmin(margin):.2f} .. {np.nanmax(margin):.2f} px^2 (median {np.nanmedian(margin):.2f})")
    assert np.isfinite(margin).all() and margin.min() > 1.0
    # the window's own arg-min agrees here: every window of a random walk has evidence
    assert np.array_equal((cost / count).argmin(axis=2) - sc.MAX_LAG, pair_lag)
    # the implementation's host part is the oracle's
    mine = sync.sync_camera_lags(np.array(pairs), pair_lag, count, 7)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(mine, (got, status, inc)))


def _count_table(pair_lag, weights, D=2):
    """count [npair, nW, 2 D + 1] with weights[k][w] at the chosen lag and 1 elsewhere."""
    pair_lag = np.asarray(pair_lag)
    count = np.ones(pair_lag.shape + (2 * D + 1,), dtype=np.int64)
    for k in range(pair_lag.shape[0]):
        for w in range(pair_lag.shape[1]):
            count[k, w, pair_lag[k, w] + D] = weights[k][w]
    return count


def _both(pairs, pair_lag, count, ncam):
    want = so.camera_lags(pairs, pair_lag, count, ncam)
    got = sync.sync_camera_lags(np.array(pairs, dtype=np.int32).reshape(-1, 2), np.asarray(pair_lag), count, ncam)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    return [a.tolist() for a in got]


def test_camera_lags_tree_gauge_and_ties():
    tri = [(0, 1), (0, 2), (1, 2)]
    # a closed triangle: camera 1 late by 2; the two good cameras are the majority
    d = [[2], [0], [-2]]
    assert _both(tri, d, _count_table(d, [[9], [9], [9]]), 3) == [[[0], [2], [0]], [1, 2, 1], [[0], [0], [0]]]
    # an open triangle: the lightest pair is left out of the tree and carries the inconsistency
    d = [[1], [0], [0]]
    assert _both(tri, d, _count_table(d, [[5], [9], [9]]), 3) == [[[0], [0], [0]], [1, 1, 1], [[1], [0], [0]]]
    assert _both(tri, d, _count_table(d, [[9], [5], [9]]), 3) == [[[-1], [0], [0]], [2, 1, 1], [[0], [-1], [0]]]
    # equal weights: the tree takes the lower (a, b), so (1, 2) is left out
    assert _both(tri, d, _count_table(d, [[9], [9], [9]]), 3) == [[[0], [1], [0]], [1, 2, 1], [[0], [0], [1]]]
    # the gauge: two cameras one frame apart tie on frequency; the smaller (|l|, l) is 0 in both, so the lag goes to the higher camera, and
    # with a negative lag the same
    assert _both([(0, 1)], [[1]], _count_table([[1]], [[9]]), 2) == [[[0], [1]], [1, 2], [[0]]]
    assert _both([(0, 1)], [[-1]], _count_table([[-1]], [[9]]), 2) == [[[0], [-1]], [1, 2], [[0]]]
    # three distinct lags 0, -1, +1: all tie on frequency, and (|l|, l) takes 0; with -1, +1 and +2 it takes -1
    chain = [(0, 1), (1, 2)]
    d = [[-1], [2]]
    assert _both(chain, d, _count_table(d, [[9], [9]]), 3)[0] == [[0], [-1], [1]]
    d = [[1], [1]]   # lags 0, 1, 2 before the gauge
    assert _both(chain, d, _count_table(d, [[9], [9]]), 3)[0] == [[0], [1], [2]]
    d = [[-1], [-1]]   # 0, -1, -2
    assert _both(chain, d, _count_table(d, [[9], [9]]), 3)[0] == [[0], [-1], [-2]]
    # two components and a camera alone; the lag changes between the windows; status 2 needs one window only
    pairs = [(0, 2), (3, 4)]
    d = [[0, 0], [0, 2]]
    lag, status, inc = _both(pairs, d, _count_table(d, [[9, 9], [9, 9]]), 5)
    assert lag == [[0, 0], [0, 0], [0, 0], [0, 0], [0, 2]] and status == [1, 0, 1, 1, 2] and inc == [[0, 0], [0, 0]]
    # no pair at all, and no window
    assert _both([], np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3, 5), dtype=np.int64), 3) == [[[0] * 3] * 3, [0, 0, 0], []]
    assert _both(tri, np.zeros((3, 0), dtype=np.int64), np.zeros((3, 0, 5), dtype=np.int64), 3)[:2] == [[[], [], []], [1, 1, 1]]


def test_oracle_paths_rules():
    """The Viterbi's tie rules on hand-made tables (tests/test_gpu_sync.py runs the same tables on the device)."""
    ten = lambda rows: np.full((1, len(rows), len(rows[0])), 10, dtype=np.int64)   # noqa: E731
    run = lambda rows, kq, m=1: so.paths(np.array([rows], dtype=np.int64), ten(rows), kq, m)   # noqa: E731
    assert run([[5] * 5] * 4, 1024)[0].tolist() == [[0, 0, 0, 0]]
    assert run([[9, 3, 9, 3, 9]], 0)[0].tolist() == [[-1]] and run([[3, 9, 9, 3, 9]], 0)[0].tolist() == [[1]]
    assert run([[7] * 5, [50, 50, 50, 50, 0]], 0)[0].tolist() == [[0, 2]]
    assert run([[7] * 5, [50, 50, 50, 50, 0]], 1024)[0].tolist() == [[2, 2]]
    lag, total, _ = run([[90, 0, 5, 0, 90], [90, 90, 0, 90, 90]], 1)   # predecessors -1 and +1 tie at 1, 0 costs 5
    assert lag.tolist() == [[-1, 0]] and total.tolist() == [1]
    rows = [[900, 900, 900, 0, 900], [4, 4, 4, 4, 4], [900, 900, 900, 0, 900]]
    assert run(rows, 64 * 1024)[0].tolist() == [[1, 1, 1]] and run(rows, 0)[0].tolist() == [[1, 0, 1]]
    margin = run([[1024 * 10 * 3, 1024 * 10 * 1, 1024 * 10 * 7]], 0)[2]
    assert margin.tolist() == [[2.0]]
    assert np.isnan(run([[3, 1, 7]], 0, 11)[2]).all()


def test_oracle_sample_rules():
    """The sample's validity and truncation: F = [0 0 0; 0 0 -3; 0 4 0] makes s = 4 row_a - 3 row_b and the denominator 25."""
    F = np.array([0, 0, 0, 0, 0, -3, 0, 4, 0], dtype=np.float64)
    pa = np.array([(3.25, 11.0), (4.0, 12.0), (7.0, 13.0), (0.0, 5.0), (5.0, 0.0), (4.0, 12.0)])
    pb = np.array([(2.0, 5.0), (2.0, 6.0), (2.0, 7.0), (2.0, 5.0), (2.0, 5.0), (0.0, 6.0)])
    q, valid = so.sample_costs(F, pa, pb, 2.0)
    assert valid.tolist() == [True, True, True, False, False, False] and q.tolist() == [2007, 4096, 4096, 0, 0, 0]
    assert not so.sample_costs(np.zeros(9), pa, pb, 2.0)[1].any()
    q, valid = so.sample_costs(F, np.array([(NAN, 3.0)]), np.array([(2.0, 5.0)]), 2.0)   # a NaN costs tau^2
    assert valid.tolist() == [True] and q.tolist() == [4096]


def test_parameters_and_refusals():
    from deepfly3d_amd import config as cfg

    assert sync.sync_params() == (cfg.SYNC_MAX_LAG, cfg.SYNC_WINDOW, cfg.SYNC_TAU, cfg.SYNC_SWITCH, cfg.SYNC_MIN_COUNT) == (8, 256, 20.0, 64.0, 16)
    assert sync.sync_params(0, 1, 0, 0.0, 1) == (0, 1, 0.0, 0.0, 1) and sync.sync_params(np.int64(64), tau=np.float32(4096.0))[::2] == (64, 4096.0, 16)
    for kw, text in (({"max_lag": -1}, "max_lag must be an integer"), ({"max_lag": 65}, "max_lag must be an integer"),
                     ({"max_lag": 2.0}, "max_lag must be an integer"), ({"max_lag": True}, "max_lag must be an integer"),
                     ({"window": 0}, "window must be an integer"), ({"window": 1.5}, "window must be an integer"),
                     ({"tau": -1.0}, "tau must be in"), ({"tau": NAN}, "tau must be in"), ({"tau": 5000.0}, "tau must be in"),
                     ({"tau": "3"}, "tau must be a number"), ({"switch": -1.0}, "switch must be in"), ({"switch": NAN}, "switch must be in"),
                     ({"switch": float("inf")}, "switch must be in"), ({"min_count": 0}, "min_count must be an integer"),
                     ({"min_count": 2.5}, "min_count must be an integer")):
        with pytest.raises(ValueError, match=text):
            sync.sync_params(**kw)
    # the host entries refuse their arguments before any device work
    count = np.ones((1, 2, 5), dtype=np.int64)
    for args, text in ((([(0, 1)], np.zeros((2, 2), dtype=np.int64), count, 2), "pair_lag must be"),
                       (([(0, 1)], np.zeros((1, 2), dtype=np.int64), count[:, :, :4], 2), "pair_lag must be"),
                       (([(0, 1)], np.full((1, 2), 3), count, 2), r"pair_lag must lie in \[-2, 2\]"),
                       (([(0, 2)], np.zeros((1, 2), dtype=np.int64), count, 2), "pairs must hold distinct cameras")):
        with pytest.raises(ValueError, match=text):
            sync.sync_camera_lags(*args)
    with pytest.raises(ValueError, match=r"points2d_px must be \[ncam, T, J, 2\]"):
        sync.sync_pairs(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="min_count must be"):
        sync.sync_pairs(np.zeros((2, 3, 4, 2)), 0)
    assert sync.sync_pairs(np.zeros((2, 0, 4, 2))).shape == (0, 2) and sync.sync_pairs(np.ones((3, 2, 1, 2)), 2).tolist() == [[0, 1], [0, 2], [1, 2]]
    one_zero = np.ones((2, 4, 1, 2))
    one_zero[1, :2, 0, 1] = 0.0   # a zero coordinate is no detection: two common frames are left
    assert sync.sync_pairs(one_zero, 2).tolist() == [[0, 1]] and sync.sync_pairs(one_zero, 3).shape == (0, 2)
    with pytest.raises(ValueError, match="points2d_px must be a contiguous"):
        sync.sync_pair_costs(np.zeros((2, 3, 4, 2)), np.zeros((0, 9)), [])
    with pytest.raises(ValueError, match="points2d_px must be a contiguous"):
        sync.apply_sync(np.zeros((2, 3, 4, 2)), np.zeros((2, 1), dtype=np.int32))
    with pytest.raises(ValueError, match="points2d_px must be a contiguous"):
        sync.camera_sync(sc.cameras(), np.zeros((7, 3, 4, 2)))
    with pytest.raises(ValueError, match="max_lag must be"):   # before the detections are looked at
        sync.camera_sync(None, None, max_lag=99)
    with pytest.raises(ValueError, match="cost must be a contiguous"):
        sync.sync_paths(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)))
    assert list(inspect.signature(sync.camera_sync).parameters) == ["P", "points2d_px", "max_lag", "window", "tau", "switch", "min_count"]


def test_cabi_refusals(native_lib):
    """Every argument the three entries refuse, before the device is touched (no GPU here: a call that got further would fail otherwise)."""
    import ctypes

    lib = native_lib
    F = (ctypes.c_double * 9)(*([0.0] * 9))
    pair = (ctypes.c_int * 2)(0, 1)
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    a, b, c, d, e = (base + k * 8192 for k in range(5))

    def refused(rc, text):
        assert rc == -1 and re.search(text, lib.df3d_last_error().decode()), (rc, lib.df3d_last_error())

    costs = lambda **kw: lib.df3d_sync_pair_costs(*[kw.get(k, v) for k, v in (   # noqa: E731
        ("F", F), ("pairs", pair), ("npair", 1), ("pts", a), ("ncam", 2), ("T", 4), ("J", 3), ("D", 1), ("W", 2), ("tau", 20.0), ("cost", b),
        ("count", c), ("stream", None))])
    for kw, text in (({"ncam": 0}, "ncam must be"), ({"ncam": 9}, "ncam must be"), ({"J": 0}, "J must be"), ({"J": 65}, "J must be"),
                     ({"T": -1}, "T must be"), ({"T": (1 << 20) + 1}, "T must be"), ({"W": 0}, "window must be"), ({"npair": -1}, "npair must be"),
                     ({"npair": 29}, "npair must be"), ({"D": -1}, "max_lag must be"), ({"D": 65}, "max_lag must be"),
                     ({"tau": -1.0}, "tau must be"), ({"tau": NAN}, "tau must be"), ({"tau": 4097.0}, "tau must be"),
                     ({"F": None}, "null pointer: F_host"), ({"pairs": None}, "null pointer: pairs_host"),
                     ({"pairs": (ctypes.c_int * 2)(1, 1)}, "a pair must hold"), ({"pairs": (ctypes.c_int * 2)(0, 2)}, "a pair must hold"),
                     ({"pts": None}, "null pointer: pts_px"), ({"cost": None}, "null pointer: cost"), ({"count": b + 4}, "count must be 8-byte aligned"),
                     ({"count": b}, "count must not overlap cost"), ({"cost": a + 8}, "cost must not overlap pts_px")):
        refused(costs(**kw), text)
    assert costs(T=0, pts=None, cost=None, count=None) == 0 and costs(npair=0, pts=None, cost=None, count=None, F=None, pairs=None) == 0

    need = lib.df3d_sync_work_bytes(1, 2, 1)
    assert need >= 6 and lib.df3d_sync_work_bytes(29, 2, 1) == 0 and lib.df3d_sync_work_bytes(1, -1, 1) == 0 and lib.df3d_sync_work_bytes(1, 2, 65) == 0
    paths = lambda **kw: lib.df3d_sync_paths(*[kw.get(k, v) for k, v in (   # noqa: E731
        ("cost", a), ("count", b), ("npair", 1), ("nW", 2), ("D", 1), ("kq", 5), ("min_count", 1), ("lag", c), ("path_cost", c + 64), ("margin", d),
        ("work", e), ("work_bytes", need), ("stream", None))])
    for kw, text in (({"npair": 29}, "npair must be"), ({"D": 65}, "max_lag must be"), ({"nW": -1}, "number of windows"),
                     ({"nW": (1 << 20) + 1}, "number of windows"), ({"kq": -1}, "switch cost"), ({"kq": (1 << 34) + 1}, "switch cost"),
                     ({"min_count": -1}, "min_count must be"), ({"work_bytes": need - 1}, "work buffer too small"), ({"cost": None}, "null pointer: cost"),
                     ({"lag": c + 2}, "lag must be 4-byte aligned"), ({"margin": a}, "margin must not overlap cost"),
                     ({"work": None}, "null pointer: work"), ({"path_cost": c}, "path_cost must not overlap lag")):
        refused(paths(**kw), text)
    assert paths(nW=0, cost=None) == 0 and paths(npair=0, cost=None) == 0

    apply = lambda **kw: lib.df3d_sync_apply(*[kw.get(k, v) for k, v in (   # noqa: E731
        ("pts", a), ("lag", b), ("ncam", 2), ("T", 4), ("J", 3), ("W", 2), ("out", c), ("stream", None))])
    for kw, text in (({"ncam": 9}, "ncam must be"), ({"J": 65}, "J must be"), ({"T": -1}, "T must be"), ({"W": 0}, "window must be"),
                     ({"pts": None}, "null pointer: pts_px"), ({"lag": b + 2}, "lag_cam must be 4-byte aligned"), ({"out": a}, "out must not overlap pts_px"),
                     ({"out": None}, "null pointer: out")):
        refused(apply(**kw), text)
    assert apply(T=0, pts=None, lag=None, out=None) == 0


def _one_frame_folder(tmp_path, golden_dir):
    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    return str(folder)


def test_core_refusals_and_keys(tmp_path, golden_dir):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    assert Core._SYNC_KEYS == ("sync_lag", "sync_status", "sync_pairs", "sync_pair_lag", "sync_pair_margin", "sync_pair_inconsistency",
                               "sync_pair_cost", "sync_pair_count", "sync_params")
    save = inspect.signature(Core.save).parameters
    names = ("check_sync", "sync_cameras", "sync_max_lag", "sync_window", "sync_tau", "sync_switch", "sync_min_count")
    assert [save[n].default for n in names] == [False, False, None, None, None, None, None]
    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    with pytest.raises(RuntimeError, match="camera_sync needs calibrated cameras"):
        core.camera_sync()
    with pytest.raises(ValueError, match="max_lag must be"):   # before the cameras are asked for
        core.camera_sync(max_lag=65)
    with pytest.raises(TypeError):
        core.camera_sync(lag=3)
    for option in names[2:]:
        with pytest.raises(ValueError, match="belong to check_sync and sync_cameras"):
            core.save(**{option: 3})
    with pytest.raises(ValueError, match="window must be"):
        core.save(check_sync=True, sync_window=0)
    with pytest.raises(ValueError, match="tau must be"):
        core.save(sync_cameras=True, sync_tau=NAN)
    with pytest.raises(ValueError, match="cannot follow auto_correct"):
        core.save(sync_cameras=True, heatmap_triangulation=True)
    core._corrected = True
    with pytest.raises(ValueError, match="cannot follow auto_correct"):
        core.save(sync_cameras=True)
    core._corrected = False
    assert not [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]
    config.pop("image_shape", None)


def test_cli_options_and_refusals(capsys, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    cases = [(["x", f"--sync-{name}", "3"], f"--sync-{name} sets a parameter of --check-sync and --sync-cameras")
             for name in ("max-lag", "window", "tau", "switch")]
    cases += [(["x", "--sync-cameras", flag], f"--sync-cameras shifts the detections' frames, and {flag} reads the heat-maps by frame index")
              for flag in ("--auto-correct", "--track-2d", "--heatmap-triangulation", "--video-heatmap")]
    cases += [(["x", "--check-sync", "--sync-max-lag", "65"], r"max_lag must be an integer in \[0, 64\]"),
              (["x", "--check-sync", "--sync-window", "0"], "window must be an integer"),
              (["x", "--sync-cameras", "--sync-tau", "nan"], "tau must be in"),
              (["x", "--sync-cameras", "--sync-switch=-1"], "switch must be in")]
    for argv, message in cases:
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err), argv
    args = cli.parse_cli_args(["x", "--sync-cameras", "--sync-max-lag", "3", "--sync-window", "64", "--sync-tau", "7.5", "--sync-switch", "9",
                               "--skip-pose-estimation"])
    assert args.sync_cameras and not args.check_sync and (args.sync_max_lag, args.sync_window, args.sync_tau, args.sync_switch) == (3, 64, 7.5, 9.0)
    args = cli.parse_cli_args(["x", "--check-sync", "--auto-correct", "--video-heatmap"])   # the check alone shifts nothing
    assert args.check_sync and not args.sync_cameras
    args = cli.parse_cli_args(["x"])
    assert not args.check_sync and not args.sync_cameras and args.sync_max_lag is None and args.sync_switch is None
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--sync-max-lag N" in text and "--sync-window W" in text and "--sync-tau PX" in text and "--sync-switch K" in text
    assert "a lag between the left and the right cameras cannot be seen" in text
    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    for flag in ("--check-sync", "--sync-cameras"):
        with pytest.raises(RuntimeError, match=f"{flag} needs calibrated cameras"):
            cli.run(cli.parse_cli_args([folder, flag, "--skip-pose-estimation"]))
    config.pop("image_shape", None)
