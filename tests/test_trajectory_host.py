"""CPU tests of the trajectory triangulation's model (tests/trajectory_oracle.py) and of everything the feature
refuses before it touches a device: the oracle against independent statements of its parts, what the fit is worth on planted
trajectories (inequalities against the plain triangulation on the same input), parameters, signatures, keys and messages."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import pose_repair_oracle as pr
import trajectory_cases as tc
import trajectory_oracle as to

NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------ the oracle's parts
def test_per_point_minimiser_with_no_smoothing_and_no_huber():
    """lambda = 0 and delta = inf decouple the frames: every anchor is its own reprojection minimiser (scipy, independently)."""
    from scipy.optimize import least_squares

    P, px, _ = tc.clean(3, 12, 2)
    X0 = tc.dlt(P, px)
    r = to.fit(P, px, X0, 0.0, math.inf, 10)
    assert (r["fit_status"] == to.CONVERGED).all() and (r["status"] == 1).all() and (r["weight"][:3] == 1.0).all()

    def residual(x, t, j):
        out = []
        for c in range(3):
            u, v, w = P[c] @ np.append(x, 1.0)
            out += [u / w - px[c, t, j, 1], v / w - px[c, t, j, 0]]
        return np.array(out)

    for t, j in ((0, 0), (3, 1), (7, 0), (11, 1)):
        best = least_squares(residual, X0[t, j], args=(t, j), xtol=1e-15, ftol=1e-15, gtol=1e-15).x
        assert np.abs(r["X"][t, j] - best).max() < 1e-7, (t, j)
    assert not np.array_equal(r["X"], X0)          # the DLT does not minimise the reprojection error


def test_a_large_lambda_reproduces_affine_motion():
    """The penalty's null space: with every view on every frame an affine trajectory comes back, and any input turns affine."""
    P = tc.rig()
    T, t = 30, np.arange(30.0)[:, None, None]
    start = tc.sinusoid(1, 2)[0]
    truth = start[None] + t * np.array([[0.01, -0.02, 0.005], [-0.015, 0.0, 0.01]])[None]
    px = tc.project(P, truth)
    px[3:] = 0.0
    noise = np.random.default_rng(3).normal(0.0, 0.05, size=truth.shape)
    r = to.fit(P, px, truth + noise, 1e8, 10.0, 10)
    assert (r["fit_status"] == to.CONVERGED).all()
    assert np.abs(r["X"] - truth).max() < 1e-6
    P, px, _ = tc.clean(3, 30, 2)
    r = to.fit(P, px, tc.dlt(P, px), 1e12, 10.0, 10)
    second = r["X"][:-2] - 2.0 * r["X"][1:-1] + r["X"][2:]
    assert (r["fit_status"] == to.CONVERGED).all() and np.abs(second).max() < 1e-6


def _active_by_walk(anchor, max_gap):
    out = np.zeros(len(anchor), bool)
    for a, b in to.segments_loop(anchor, max_gap):
        out[a : b + 1] = True
    return out


def test_segment_rule_at_its_edges():
    def active(bits, max_gap):
        a = np.array([c == "1" for c in bits])
        got = to.active_frames(a[:, None], max_gap)[0][:, 0]
        assert np.array_equal(got, _active_by_walk(a, max_gap)), (bits, max_gap)
        return "".join("1" if v else "0" for v in got)

    assert active("1110111", 0) == "1110111"            # max_gap = 0 bridges nothing: two segments of three
    assert active("1101011", 0) == "0000000"            # ... and runs of fewer than three frames are copied
    assert active("1100011", 3) == "1111111"            # a gap of exactly max_gap
    assert active("1100011", 2) == "0000000"            # max_gap + 1: two runs of two frames
    assert active("11100001", 3) == "11100000"          # the long gap cuts; the lone anchor behind it is copied
    assert active("0011100", 10) == "0011100"           # a gap at either end of the recording is never bridged
    assert active("0000000", 10) == "0000000"           # no anchor
    assert active("0001000", 10) == "0000000"           # one anchor
    assert active("1000001", 5) == "1111111"            # two anchors and a bridged gap make a segment
    assert active("101", 1) == "111" and active("11", 5) == "00" and active("1", 5) == "0"
    rng = np.random.default_rng(8)
    for _ in range(200):
        a = rng.random(int(rng.integers(1, 40))) < rng.choice([0.2, 0.5, 0.9])
        for max_gap in (0, 1, 2, 5):
            assert np.array_equal(to.active_frames(a[:, None], max_gap)[0][:, 0], _active_by_walk(a, max_gap))


def test_start_points_are_fill_gaps_operations():
    P, px, _, gap = tc.one_view_gaps(60, 1, starts=(10, 30))
    X0 = tc.dlt(P, px)
    anchor = to.anchors(px, X0)
    assert np.array_equal(~anchor[:, 0], gap)
    active, _ = to.active_frames(anchor, 10)
    X38, flags = np.zeros((60, 38, 3)), np.zeros((60, 38), np.uint8)
    X38[:, :1], flags[:, 0] = X0, ~anchor[:, 0]
    assert np.array_equal(to.start_points(X0, anchor, active)[:, 0], pr.fill_gaps(X38, flags, 10)[0][:, 0])


def test_banded_solve_and_chain_sum_against_dense_statements():
    T, J = 21, 3
    H, g, X = tc.solve_terms(T, 38)
    H, g, X = H[:, :J], g[:, :J], X[:, :J]
    active = np.ones((T, J), bool)
    active[[0, 9, 20], 1] = False
    c = to.centres(active)
    lam, mu = np.array([0.0, 1e4, 1e8]), np.full(J, 1e-3)
    AB, b = to.system(H, g + lam[None, :, None] * to.smoothness(X, c)[1], c, active, lam, mu)
    x, ok = to.banded_solve(AB, b)
    A = to.dense(AB)
    assert ok.all() and np.array_equal(A, A.transpose(0, 2, 1))
    for j in range(J):
        assert np.linalg.eigvalsh(A[j]).min() > 0.0
        want = np.linalg.solve(A[j], b[j])
        assert np.abs(x[j] - want).max() <= 1e-9 * np.abs(want).max()
        # K is the Gram matrix of the second differences of the segments: x^T (A - H - mu I) x = lam sum |s|^2
        v = np.random.default_rng(j).normal(size=(T, 1, 3))
        s = to.smoothness(v, c[:, j : j + 1])[0]
        quad = v.reshape(-1) @ (A[j] @ v.reshape(-1))
        Hq = sum(float(v[t, 0] @ np.array([[H[t, j, 0], H[t, j, 1], H[t, j, 2]], [H[t, j, 1], H[t, j, 3], H[t, j, 4]],
                                             [H[t, j, 2], H[t, j, 4], H[t, j, 5]]]) @ v[t, 0]) + mu[j] * float(v[t, 0] @ v[t, 0])
                 if active[t, j] else float(v[t, 0] @ v[t, 0]) for t in range(T))
        assert abs(quad - Hq - lam[j] * float((s ** 2).sum())) <= 1e-9 * abs(quad)
    assert to.backward_error(AB, b, x).max() < 1e-14
    f = np.random.default_rng(1).random((600, 2))
    assert np.allclose(to.chain_sum(f), f.sum(axis=0), rtol=1e-13) and np.array_equal(to.chain_sum(f[:1]), f[0])


def test_gradient_and_huber_against_finite_differences():
    P, px, _, _ = tc.outliers(3, 20, 1)
    X = tc.dlt(P, px) + 0.01
    for delta in (2.0, 10.0, math.inf):
        H, g, w, e, cost = to.linearize(P, px, X, delta)
        assert ((w == 1.0) == (e <= delta))[:3].all() and (w[3:] == 0.0).all() and (e[3:] == 0.0).all()
        for k in range(3):
            h = np.zeros(3)
            h[k] = 1e-6
            up, down = to.linearize(P, px, X + h, delta)[4], to.linearize(P, px, X - h, delta)[4]
            assert np.allclose((up - down) / 2e-6, 2.0 * g[..., k], rtol=1e-5, atol=1e-4)      # d rho / dX = 2 w J^T r


# --------------------------------------------------------------------------------------------------- what the fit is worth (oracle alone)
def _fit(P, px):
    X0 = tc.dlt(P, px)
    r = to.fit(P, px, X0, tc.LAMBDA, tc.HUBER, 10)
    assert (r["fit_status"] == to.CONVERGED).all()
    return X0, r


def test_value_a_one_view_frames_beat_interpolation():
    P, px, truth, gap = tc.one_view_gaps()
    X0, r = _fit(P, px)
    X38, flags = np.zeros((400, 38, 3)), np.zeros((400, 38), np.uint8)
    X38[:, :1], flags[:, 0] = X0, gap
    filled = pr.fill_gaps(X38, flags, 10)[0][:, :1]
    before, after = tc.rms(filled, truth, gap), tc.rms(r["X"], truth, gap)
    print(f"(a) one-view runs of 8 frames: interpolation {before:.4f} mm rms, the fit {after:.4f} mm")
    assert (r["status"][gap] == 2).all() and (r["status"][~gap] == 1).all()
    assert after < before


@pytest.mark.parametrize("nviews", [2, 3])
def test_value_b_outliers_are_down_weighted(nviews):
    P, px, truth, planted = tc.outliers(nviews)
    X0, r = _fit(P, px)
    rows = planted.any(axis=0)[:, 0]
    before, after = tc.rms(X0, truth, rows), tc.rms(r["X"], truth, rows)
    clean = to.views(px) & ~planted.any(axis=0)[None]
    low = float((r["weight"][clean] < 1.0).mean())
    print(f"(b) {nviews} views, 60 px outliers: on their frames the plain triangulation {before:.4f} mm rms, the fit {after:.4f} mm; "
          f"clean views of clean frames below weight 1: {low:.4f}")
    assert after < before
    assert (r["weight"][planted] < 1.0).all()
    assert low <= tc.CLEAN_DOWNWEIGHTED_CAP


@pytest.mark.parametrize("nviews", [2, 3])
def test_value_c_clean_detections_are_not_made_worse(nviews):
    P, px, truth = tc.clean(nviews)
    X0, r = _fit(P, px)
    before, after = tc.rms(X0, truth), tc.rms(r["X"], truth)
    print(f"(c) {nviews} clean views: the plain triangulation {before:.4f} mm rms, the fit {after:.4f} mm")
    assert after <= before


# ------------------------------------------------------------------------------------------------------------------ host refusals
def test_kernel_constants_are_configs():
    from deepfly3d_amd import config as cfg

    text = open(os.path.join(os.path.dirname(cfg.__file__), "csrc", "trajectory.hip")).read()

    def constant(name):
        return float(re.search(rf"\b{name} = ([0-9.e+-]+)[,;]", text).group(1))

    assert constant("TOL") == cfg.TRAJECTORY_STEP_TOL and constant("SLACK") == cfg.TRAJECTORY_SLACK
    assert (constant("MU_INIT"), constant("MU_MIN"), constant("MU_MAX")) == (cfg.TRAJECTORY_MU_INIT, cfg.TRAJECTORY_MU_MIN, cfg.TRAJECTORY_MU_MAX)
    assert constant("MAX_ITER") == cfg.TRAJECTORY_MAX_ITER and constant("BLOCK_MIN") == cfg.TRAJECTORY_BLOCK_FRAMES_RANGE[0]
    assert "BLOCK_MAX = 1 << 20" in text and cfg.TRAJECTORY_BLOCK_FRAMES_RANGE[1] == 1 << 20
    assert "MAX_T = 1 << 20" in text and cfg.TRAJECTORY_MAX_FRAMES == 1 << 20


def test_trajectory_params():
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops

    l, h, gap, b = ops.trajectory_params()
    assert l.dtype == np.float64 and np.array_equal(l, cfg.TRAJECTORY_LAMBDA) and l is not cfg.TRAJECTORY_LAMBDA and l.shape == (38,)
    assert (h, gap, b) == (cfg.TRAJECTORY_HUBER, cfg.REPAIR_MAX_GAP, None)      # the block then follows the recording's length
    assert [cfg.trajectory_block_frames(T) for T in (0, 1, 9, 10, 1000, 1024, 1025, 1 << 20)] == [3, 3, 3, 4, 32, 32, 33, 1024]
    l, h, gap, b = ops.trajectory_params(5, math.inf, 0, 3)
    assert l.tolist() == [5.0] and h == math.inf and gap == 0 and b == 3
    assert ops.trajectory_params(np.arange(38.0), 0.0, np.int64(7), np.int64(64))[0].shape == (38,)
    for bad in (-1.0, NAN, math.inf, [1.0, -2.0], [1.0, NAN], [], "5", True, object(), [None]):
        with pytest.raises(ValueError, match="lam must be"):
            ops.trajectory_params(bad)
    for bad in (-1.0, NAN, "5", True, [1.0]):
        with pytest.raises(ValueError, match="huber must be"):
            ops.trajectory_params(None, bad)
    for bad in (-1, 1000001, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"max_gap must be an integer in \[0, 1000000\]"):
            ops.trajectory_params(None, None, bad)
    for bad in (2, 0, (1 << 20) + 1, 16.0, True):
        with pytest.raises(ValueError, match=r"block_frames must be an integer in \[3, 1048576\]"):
            ops.trajectory_params(None, None, None, bad)
    assert list(inspect.signature(ops.trajectory_params).parameters) == ["lam", "huber", "max_gap", "block_frames"]
    assert list(inspect.signature(ops.triangulate_trajectory).parameters) == ["P", "points2d_px", "X", "lam", "huber", "max_gap", "block_frames"]
    assert [f.name for f in ops.TrajectoryResult.__dataclass_fields__.values()] == ["points3d", "status", "weight", "error", "iterations", "cost",
                                                                                    "counts", "params"]
    assert callable(ops.trajectory_linearize) and callable(ops.trajectory_solve)


def _one_frame_folder(tmp_path, golden_dir):
    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    return str(folder)


def test_core_refusals_and_keys(tmp_path, golden_dir):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    assert Core._TRAJECTORY_KEYS == ("points3d_trajectory", "trajectory_status", "trajectory_weight", "trajectory_error", "trajectory_iterations",
                                     "trajectory_cost", "trajectory_counts", "trajectory_params")
    names = list(inspect.signature(Core.save).parameters)
    assert names[-7:] == ["trajectory_triangulation", "trajectory_lambda", "trajectory_huber", "trajectory_max_gap", "robust_triangulation",
                          "robust_tau", "robust_min_views"]
    assert [inspect.signature(Core.save).parameters[n].default for n in names[-7:-3]] == [False, None, None, None]
    assert list(inspect.signature(Core.trajectory_triangulation).parameters) == ["self", "lam", "huber", "max_gap"]
    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    with pytest.raises(RuntimeError, match="trajectory_triangulation needs calibrated cameras"):
        core.trajectory_triangulation()
    with pytest.raises(ValueError, match="lam must be"):   # before the cameras are asked for
        core.trajectory_triangulation(lam=-1.0)
    with pytest.raises(ValueError, match="huber must be"):
        core.trajectory_triangulation(huber=NAN)
    with pytest.raises(ValueError, match="max_gap must be"):
        core.trajectory_triangulation(max_gap=-1)
    for option in ("trajectory_lambda", "trajectory_huber", "trajectory_max_gap"):
        with pytest.raises(ValueError, match="trajectory_lambda, trajectory_huber and trajectory_max_gap belong to trajectory_triangulation"):
            core.save(**{option: 3})
    with pytest.raises(ValueError, match="lam must be"):
        core.save(trajectory_triangulation=True, trajectory_lambda=NAN)
    with pytest.raises(ValueError, match="huber must be"):
        core.save(trajectory_triangulation=True, trajectory_huber=-2.0)
    with pytest.raises(ValueError, match="max_gap must be"):
        core.save(trajectory_triangulation=True, trajectory_max_gap=1.5)
    with pytest.raises(ValueError, match="trajectory_lambda must hold one value, or one per joint"):
        core.save(trajectory_triangulation=True, trajectory_lambda=[1.0, 2.0])
    assert not [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]
    config.pop("image_shape", None)


def test_cli_options_and_refusals(capsys, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    needs = "sets a parameter of --trajectory-triangulation: it needs --trajectory-triangulation"
    for argv, message in ((["x", "--trajectory-lambda", "5"], "--trajectory-lambda " + needs),
                          (["x", "--trajectory-huber", "3"], "--trajectory-huber " + needs),
                          (["x", "--trajectory-max-gap", "3"], "--trajectory-max-gap " + needs),
                          (["x", "--trajectory-triangulation", "--trajectory-lambda=-1"], "lam must be >= 0 and finite"),
                          (["x", "--trajectory-triangulation", "--trajectory-lambda", "inf"], "lam must be >= 0 and finite"),
                          (["x", "--trajectory-triangulation", "--trajectory-huber", "nan"], "huber must be >= 0 and not NaN"),
                          (["x", "--trajectory-triangulation", "--trajectory-max-gap=-1"], r"max_gap must be an integer in \[0, 1000000\]")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err), argv
    args = cli.parse_cli_args(["x", "--trajectory-triangulation", "--trajectory-lambda", "1e3", "--trajectory-huber", "inf", "--trajectory-max-gap",
                               "4", "--skip-pose-estimation"])
    assert args.trajectory_triangulation and args.trajectory_lambda == 1e3 and args.trajectory_huber == math.inf and args.trajectory_max_gap == 4
    args = cli.parse_cli_args(["x"])
    assert not args.trajectory_triangulation and args.trajectory_lambda is None and args.trajectory_huber is None and args.trajectory_max_gap is None
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--trajectory-lambda L" in text and "--trajectory-huber PX" in text and "--trajectory-max-gap N" in text
    assert "The defaults are guesses that nobody has measured on a recording" in text and "the gain over the plain triangulation is small" in text
    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    with pytest.raises(RuntimeError, match="--trajectory-triangulation needs calibrated cameras"):
        cli.run(cli.parse_cli_args([folder, "--trajectory-triangulation", "--skip-pose-estimation"]))
    config.pop("image_shape", None)
