"""CPU tests of the constant-length leg fit: the float64 oracle tests/leg_fit_oracle.py against an independent
scipy fit and against its own properties (convergence, exact lengths, the replay's cost, rigid input, the legs that are not fitted,
the other tangent basis), the argument validation of df3d_leg_fit (no device is touched), ops' argument errors, the CLI flag and
Core.rigid_legs' refusals."""
import ctypes
import os

import numpy as np
import pytest

import leg_fit_oracle as lo

WITNESS_TOL = 1e-6        # mm: scipy's stopping precision with a margin (measured: 1.8e-9 golden, 1.6e-9 synthetic)
WITNESS_COST_RTOL = 1e-9
LENGTH_RTOL = 1e-12       # differences of coordinates of up to ten segment lengths
RIGID_COST = 1e-24        # mm^2


@pytest.fixture(scope="module")
def sets(golden_dir):
    """{name: (X, lengths, anchor, the oracle's fit, the max_iter = 0 replay)} for the golden recording with its median lengths and
    for 40 seeded synthetic flies with the same lengths, noise of 0.02 x the mean length and an offset anchor; computed once."""
    X = np.load(f"{golden_dir}/golden_3d.npz")["points3d_wo_procrustes"]
    L = lo.median_lengths(X)
    Xs, A, _ = lo.synthetic_flies(np.random.default_rng(15), 40, L)
    out = {}
    for name, (Y, anchor) in {"golden": (X, None), "synthetic": (Xs, A)}.items():
        fit, replay = lo.fit_legs(Y, L, anchor), lo.fit_legs(Y, L, anchor, max_iter=0)
        for a in (Y, L) + fit + replay:
            a.setflags(write=False)
        out[name] = (Y, L, anchor, fit, replay)
    return out


# ------------------------------------------------------------------------------------------------------------------ the oracle
def test_golden_lengths_vary_as_the_design_says(sets):
    X = sets["golden"][0]
    sl = lo.segment_lengths(X)
    cv = sl.std(axis=0) / sl.mean(axis=0)
    assert sl.shape == (15, 6, 4) and 0.014 < cv.min() < 0.016 and 0.076 < cv.max() < 0.078   # 1.5 % .. 7.7 %


@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_oracle_agrees_with_the_scipy_witness(sets, name):
    X, L, anchor, (pts, cost, status, _), _ = sets[name]
    worst, worst_cost = 0.0, -np.inf
    for t in range(len(X)):
        for leg in range(6):
            j = lo.leg_joints(leg)
            w, Ew = lo.witness_fit(X[t, j], L[leg], None if anchor is None else anchor[leg])
            worst = max(worst, float(np.abs(w - pts[t, j]).max()))
            worst_cost = max(worst_cost, cost[t, leg] / Ew - 1.0)
            assert cost[t, leg] <= Ew * (1.0 + WITNESS_COST_RTOL), (t, leg)   # no leg excluded: the witness is never better
    print(f"{name}: oracle against the witness {worst:.3e} mm, cost ratio - 1 at most {worst_cost:.3e}")
    assert worst <= WITNESS_TOL


@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_every_leg_converges_with_exact_lengths_below_the_replay(sets, name):
    X, L, anchor, (pts, cost, status, iters), (rep, rep_cost, rep_status, rep_iters) = sets[name]
    print(f"{name}: iterations {iters.min()}..{iters.max()}, mean {iters.mean():.2f}; cost {cost.mean():.3e}, replay {rep_cost.mean():.3e} mm^2 per leg")
    assert (status == lo.CONVERGED).all() and (iters >= 1).all() and (iters < 30).all()
    assert (rep_status == lo.OUT_OF_ITERATIONS).all() and (rep_iters == 0).all()
    got = lo.segment_lengths(pts)
    assert np.abs(got / L - 1.0).max() <= LENGTH_RTOL and np.abs(lo.segment_lengths(rep) / L - 1.0).max() <= LENGTH_RTOL
    assert (cost <= rep_cost).all()
    if name == "golden":
        assert (cost < rep_cost).all()
        assert abs(cost.mean() - 2.6e-3) < 1e-4 and abs(rep_cost.mean() - 7.1e-3) < 1e-4   # the issue's table
        move = np.sqrt(((pts - X) ** 2).sum(axis=-1))
        assert 0.15 < move.max() < 0.17
    # the cost is what it says: the summed squared distance of joints 1..4, and joint 0 is the anchor
    for t in range(len(X)):
        for leg in range(6):
            j = lo.leg_joints(leg)
            assert abs(((pts[t, j[1:]] - X[t, j[1:]]) ** 2).sum() - cost[t, leg]) <= 1e-12 * cost[t, leg] + 1e-30
            assert np.array_equal(pts[t, j[0]], X[t, j[0]] if anchor is None else anchor[leg])
    others = [j for j in range(38) if j not in [k for leg in range(6) for k in lo.leg_joints(leg)]]
    assert len(others) == 8 and np.array_equal(pts[:, others], X[:, others])


def test_max_iter_zero_is_the_closed_form_replay(sets):
    for name in ("golden", "synthetic"):
        X, L, anchor, _, (rep, _, _, _) = sets[name]
        for t in (0, len(X) - 1):
            for leg in range(6):
                j = lo.leg_joints(leg)
                assert np.array_equal(rep[t, j], lo.replay(X[t, j], L[leg], None if anchor is None else anchor[leg]))


def test_exactly_rigid_input_comes_back(sets):
    L = sets["golden"][1]
    _, _, rigid = lo.synthetic_flies(np.random.default_rng(16), 20, L, noise=0.0)
    pts, cost, status, iters = lo.fit_legs(rigid, L)
    print(f"rigid input moves by {np.abs(pts - rigid).max():.3e} mm, cost at most {cost.max():.3e} mm^2, iterations at most {iters.max()}")
    assert (status == lo.CONVERGED).all() and cost.max() <= RIGID_COST and np.abs(pts - rigid).max() <= lo.CONVERGED_BAR


def test_basis_variant_sensitivity(sets):
    """How far the converged answer depends on the arithmetic path (recorded in DESIGN.md section 15)."""
    for name in ("golden", "synthetic"):
        X, L, anchor, (pts, cost, status, iters), _ = sets[name]
        v = lo.fit_legs(X, L, anchor, basis_variant=True)
        diff = np.abs(v[0] - pts).max()
        print(f"{name}: the other tangent basis moves the answer by {diff:.3e} mm, iterations by {np.abs(v[3] - iters).max()}")
        assert (v[2] == lo.CONVERGED).all() and 10.0 * diff <= lo.CONVERGED_BAR   # the bar covers it ten times


def test_legs_that_are_not_fitted(sets):
    X, L, _, (pts, _, _, _), _ = sets["golden"]
    anchor = lo.recording_anchor(X)
    P = X[2, lo.leg_joints(4)]
    values = {"zeros": [0.0, 0.0, 0.0], "NaN": [1.0, np.nan, 2.0], "inf": [-np.inf, 3.0, 1.0]}
    for k in range(5):
        for tag, value in values.items():
            Q = P.copy()
            Q[k] = value
            out, cost, status, iters = lo.fit_leg(Q, L[4])
            assert status == lo.NOT_FITTED and iters == -1 and np.isnan(cost), (k, tag)
            assert out.tobytes() == Q.tobytes(), (k, tag)   # the input's bits
            out, cost, status, iters = lo.fit_leg(Q, L[4], anchor[4])
            if k == 0:   # the anchor stands in for a missing body-coxa joint
                want = lo.fit_leg(P, L[4], anchor[4])
                assert status == lo.CONVERGED and np.array_equal(out, want[0]) and cost == want[1], tag
            else:
                assert status == lo.NOT_FITTED and iters == -1 and np.isnan(cost) and out.tobytes() == Q.tobytes(), (k, tag)
    for bad in (np.nan, np.inf):
        a = anchor[4].copy()
        a[1] = bad
        out, cost, status, iters = lo.fit_leg(P, L[4], a)
        assert status == lo.NOT_FITTED and iters == -1 and np.isnan(cost) and np.array_equal(out, P)
    # coincident joints: a measured segment of no length has no direction
    for k in range(1, 5):
        Q = P.copy()
        Q[k] = Q[k - 1]
        assert lo.fit_leg(Q, L[4])[2] == lo.NOT_FITTED
    Q = P.copy()
    Q[1] = anchor[4]
    assert lo.fit_leg(Q, L[4], anchor[4])[2] == lo.NOT_FITTED and lo.fit_leg(Q, L[4])[2] == lo.CONVERGED
    # ... and the bound is relative: 1e-18 of the largest squared target
    Q = P.copy()
    Q[3] = Q[2] + np.array([2e-9, 0.0, 0.0]) * np.sqrt(((Q[1:] - Q[0]) ** 2).sum(axis=1).max())
    assert lo.fit_leg(Q, L[4])[2] != lo.NOT_FITTED
    Q[3] = Q[2] + np.array([0.5e-9, 0.0, 0.0]) * np.sqrt(((Q[1:] - Q[0]) ** 2).sum(axis=1).max())
    assert lo.fit_leg(Q, L[4])[2] == lo.NOT_FITTED
    # a pose with a defect: the other legs are what they were
    Y = X.copy()
    Y[2, lo.leg_joints(4)[2]] = 0.0
    out = lo.fit_legs(Y[2:3], L)
    rest = [j for leg in range(6) if leg != 4 for j in lo.leg_joints(leg)]
    assert np.array_equal(out[0][0, rest], pts[2, rest]) and out[2][0, 4] == lo.NOT_FITTED


def test_median_lengths_skip_missing_joints(sets):
    X, L = sets["golden"][:2]
    Y = X.copy()
    Y[0, 7] = 0.0          # leg 1's femur-tibia joint in frame 0: its femur and tibia do not count there
    Y[1, 7, 2] = np.nan
    M = lo.median_lengths(Y)
    sl = lo.segment_lengths(X)
    assert np.array_equal(M[1, 1], np.median(sl[2:, 1, 1])) and np.array_equal(M[1, 2], np.median(sl[2:, 1, 2]))
    keep = np.ones((6, 4), dtype=bool)
    keep[1, 1:3] = False
    assert np.array_equal(M[keep], L[keep])


# ------------------------------------------------------------------------------------------------------------------ the C entry
def test_entry_validates_arguments_without_gpu(native_lib):
    lib = native_lib
    assert hasattr(lib, "df3d_leg_fit")
    err = lib.df3d_last_error
    base = 1 << 20
    pts, out, cost, info = (ctypes.c_void_p(base + k * (1 << 16)) for k in range(4))   # T = 4: 3 648 + 3 648 + 192 + 192 bytes
    L = np.full((6, 4), 0.5)
    A = np.zeros((6, 3))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def call(pts=pts, T=4, lengths=L, anchor=None, max_iter=30, out=out, cost=cost, info=info):
        return lib.df3d_leg_fit(pts, T, None if lengths is None else ptr(lengths), None if anchor is None else ptr(anchor), max_iter, out, cost, info, None)

    # no frames: nothing to do, whatever the pointers, and no device is needed
    assert lib.df3d_leg_fit(None, 0, None, None, 30, None, None, None, None) == 0
    assert call(T=-1) == -1 and b"T must be >= 0" in err()
    assert call(max_iter=-1) == -1 and b"max_iter must be >= 0" in err()
    assert call(T=0, max_iter=-1) == -1 and b"max_iter" in err()
    for name in ("pts", "lengths", "out", "cost", "info"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    for bad in (0.0, -0.25, np.nan, np.inf):
        M = L.copy()
        M[4, 2] = bad
        assert call(lengths=M) == -1 and b"leg 4, segment 2" in err(), bad
    for bad in (np.nan, -np.inf):
        B = A.copy()
        B[3, 1] = bad
        assert call(anchor=B) == -1 and b"anchor of leg 3" in err(), bad
    nbytes = 4 * 38 * 3 * 8
    # out: a partial overlap with the poses at either end is refused (out == pts, in place, would launch: tested on the GPU)
    for o in (base + 8, base + nbytes - 8, base - nbytes + 8):
        assert call(out=ctypes.c_void_p(o)) == -1 and b"out must be pts itself" in err(), o
    for o in (base, base + nbytes - 8, base - 4 * 48 + 8, out.value, out.value + nbytes - 8):
        assert call(cost=ctypes.c_void_p(o)) == -1 and b"cost must not overlap" in err(), o
        assert call(info=ctypes.c_void_p(o)) == -1 and b"info must not overlap" in err(), o
    assert call(info=ctypes.c_void_p(cost.value + 4 * 48 - 8)) == -1 and b"each other" in err()
    assert call(info=ctypes.c_void_p(info.value + 4)) == -1 and b"8-byte aligned" in err()


# ------------------------------------------------------------------------------------------------------------------ ops, CLI, config, Core
def test_ops_argument_errors(native_lib):
    import torch

    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops

    assert cfg.RIGID_LEGS_MAX_ITER == 30 == lo.MAX_ITER
    X = torch.zeros((3, 38, 3), dtype=torch.float64)   # on the host: refused, but only after the options have been checked
    for kw in ({"lengths": "median"}, {"anchor": "thorax"}, {"max_iter": -1}, {"lengths": np.ones((6, 3))}, {"lengths": np.ones((4, 6))},
               {"anchor": np.zeros((6, 4))}, {"anchor": np.zeros(3)}, {"lengths": [["a"] * 4] * 6}):
        with pytest.raises(ValueError, match="lengths|anchor|max_iter"):
            ops.fit_legs(X, **kw)
    with pytest.raises(ValueError, match="points3d"):
        ops.fit_legs(X)
    with pytest.raises(ValueError, match="points3d"):
        ops.segment_length_medians(X)
    res = ops.LegFitResult(1, 2, 3, 4, 5)
    assert (res.points, res.cost, res.status, res.iters, res.lengths) == (1, 2, 3, 4, 5)


def test_cli_rigid_legs_flag_parses_and_counts_as_something_to_do(tmp_path, monkeypatch):
    from deepfly3d_amd import cli

    assert cli.parse_cli_args(["/tmp/x", "--rigid-legs"]).rigid_legs is True
    assert cli.parse_cli_args(["/tmp/x"]).rigid_legs is False
    args = cli.parse_cli_args(["/tmp/x", "--rigid-legs", "--joint-angles", "--skip-pose-estimation"])
    assert args.rigid_legs and args.joint_angles and args.skip_estimation
    # the early return: --skip-pose-estimation alone has nothing to do and never builds a Core; with --rigid-legs it does

    class Reached(Exception):
        pass

    def core(*a, **kw):
        raise Reached()

    monkeypatch.setattr(cli, "Core", core)
    assert cli.run(cli.parse_cli_args([str(tmp_path), "--skip-pose-estimation"])) == 0
    with pytest.raises(Reached):
        cli.run(cli.parse_cli_args([str(tmp_path), "--skip-pose-estimation", "--rigid-legs"]))


def test_cli_rigid_legs_without_a_result_to_reopen_is_refused(tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    config.pop("image_shape", None)
    args = cli.parse_cli_args([str(folder), "--rigid-legs", "--skip-pose-estimation"])
    with pytest.raises(RuntimeError, match="--rigid-legs needs calibrated cameras"):
        cli.run(args)
    config.pop("image_shape", None)
    assert not [f for f in os.listdir(str(folder) + "_df3d") if f.startswith("df3d_result")]


class _Net:
    def __init__(self, calibrated):
        self.calibrated, self.points3d = calibrated, None

    def has_calibration(self):
        return self.calibrated


def test_core_rigid_legs_needs_cameras_and_rank_zero(monkeypatch):
    from deepfly3d_amd import distributed as dd
    from deepfly3d_amd.core import Core

    core = Core.__new__(Core)
    core.camNet, core.device, core.is_primary = _Net(False), "cpu", True
    for call in (core.rigid_legs, lambda: core.joint_angles(rigid=True)):
        core.camNet = _Net(False)
        with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
            call()
        core.camNet = None
        with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
            call()
    core.camNet = _Net(True)
    monkeypatch.setattr(dd, "current", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="rigid_legs is a rank-0"):
        core.rigid_legs()
    with pytest.raises(RuntimeError, match="rank-0"):
        core.joint_angles(rigid=True)
