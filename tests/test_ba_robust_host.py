"""CPU checks of the robust-loss bundle adjustment: the float64 model (tests/ba_robust_oracle.py) against scipy's
own loss functions and against scipy.optimize.least_squares, every condition tests/test_gpu_ba_robust.py relies on (the inputs of the
kernel-level test, the robustness of the whole solves' decisions, the input conditions of the outcome test), the argument checks of the
new C entries, and the CLI / config surface.  Nothing here needs a device."""
import ctypes

import numpy as np
import pytest

import ba_cases as bc
import ba_robust_cases as brc
import ba_robust_oracle as bro
from oracle import geometry as og
from oracle.trf_lsmr import eval_blocks

EPS = np.finfo(np.float64).eps


# ---- the rho table against scipy's -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f_scale", (0.5, 2.0, 5.0))
@pytest.mark.parametrize("loss", brc.ROBUST)
def test_closed_forms_are_scipys(loss, f_scale):
    """rho, rho' and the closed-form s^2 against scipy's construct_loss_function and scale_for_robust_loss_function, away from the clamp
    (|s^2| > 1e-6: nearer to it scipy's own value is a difference of almost equal numbers)."""
    from scipy.optimize._lsq.common import scale_for_robust_loss_function
    from scipy.optimize._lsq.least_squares import construct_loss_function

    rng = np.random.default_rng(5)
    f = np.concatenate([rng.normal(0.0, 0.5, 400), rng.normal(0.0, 10.0, 400), [0.0, f_scale, -f_scale, 0.999 * f_scale, 1.001 * f_scale]])
    m = f.size
    z = (f / f_scale) ** 2
    rho = construct_loss_function(m, loss, f_scale)(f).copy()          # rho[0] = C^2 rho, rho[1] = rho', rho[2] = rho'' / C^2
    assert np.allclose(rho[0], f_scale**2 * bro.rho(loss, z), rtol=1e-14, atol=0)
    assert np.allclose(rho[1], bro.weight(loss, z), rtol=1e-14, atol=0)
    cost = construct_loss_function(m, loss, f_scale)(f, cost_only=True)
    assert abs(cost - bro.robust_cost(loss, f, f_scale)) <= 1e-14 * cost
    s2_scipy = rho[1] + 2 * rho[2] * f**2
    s2 = bro.s2_closed(loss, z)
    away = np.abs(s2) > 1e-6
    assert away.sum() > 100            # (huber beyond z = 1 is the clamp itself)
    assert np.abs(s2_scipy - s2)[away].max() <= 8 * EPS                 # absolute: scipy's sum cancels, the terms are at most 1
    if loss == "huber":
        assert np.array_equal(s2[z > 1], np.full(int((z > 1).sum()), EPS)) and (np.abs(s2_scipy[z > 1]) < 4 * EPS).all()   # noise around 0
    # scipy's scaling of (J, f) on the rows it does not clamp and we do not either
    J = rng.normal(size=(m, 3))
    Js, fs = scale_for_robust_loss_function(J.copy(), f.copy(), rho)
    _, w, s, clamped = bro.row_scale(loss, f, f_scale)
    keep = away & ~clamped
    assert np.allclose(Js[keep], J[keep] * s[keep, None], rtol=1e-9, atol=0) and np.allclose(fs[keep], (f * w / s)[keep], rtol=1e-9, atol=0)
    assert np.array_equal(s[clamped], np.full(int(clamped.sum()), np.sqrt(EPS)))


def _scipy_solve(pr, loss, f_scale):
    """least_squares in the reference's configuration with the analytic block Jacobian as a sparse matrix."""
    from scipy.optimize import least_squares
    from scipy.sparse import csr_matrix

    ncam, npts, cam_idx, pt_idx, obs_xy, intr = pr["ncam"], pr["npts"], pr["cam_idx"], pr["pt_idx"], pr["obs_xy"], pr["intr"]
    n = cam_idx.size
    rows = np.repeat(np.arange(2 * n), 9)
    cols = np.repeat(np.concatenate([(cam_idx * 6)[:, None] + np.arange(6), (6 * ncam + pt_idx * 3)[:, None] + np.arange(3)], axis=1), 2, axis=0).ravel()

    def jac(x):
        _, Jc, Jp = eval_blocks(x, ncam, intr, cam_idx, pt_idx, obs_xy)
        return csr_matrix((np.concatenate([Jc, Jp], axis=2).reshape(2 * n, 9).ravel(), (rows, cols)), shape=(2 * n, 6 * ncam + 3 * npts))

    return least_squares(lambda x: og.ba_residuals(x, ncam, intr, cam_idx, pt_idx, obs_xy), pr["x0"], jac=jac, method="trf", tr_solver="lsmr", x_scale="jac",
                         ftol=1e-4, loss=loss, f_scale=f_scale)


@pytest.mark.parametrize("fraction", (0.0, 0.05))
@pytest.mark.parametrize("f_scale", (2.0, 5.0))
@pytest.mark.parametrize("name", ("three", "eight_1032"))
def test_oracle_is_scipys_solver(name, f_scale, fraction):
    """The same nfev and status as scipy.optimize.least_squares(loss='soft_l1'), the cost within 1e-9: the bar oracle/trf_lsmr.py meets
    for the linear loss."""
    case = bc.make_case(name)
    px, _ = brc.plant(name, fraction, 40.0, 41)
    pr = bro.problem(px, case["R_init"], case["tvec_init"], case["intr"])
    ref = _scipy_solve(pr, "soft_l1", f_scale)
    got = bro.trf_lsmr_robust(pr["evaluate"], pr["x0"], "soft_l1", f_scale)
    print("%s f_scale %g outliers %g: scipy nfev %d status %d cost %.12g; oracle nfev %d status %d cost %.12g"
          % (name, f_scale, fraction, ref.nfev, ref.status, ref.cost, got["nfev"], got["status"], got["cost"]))
    assert (got["nfev"], got["status"]) == (ref.nfev, ref.status)
    assert abs(got["cost"] - ref.cost) <= 1e-9 * ref.cost


def test_linear_oracle_is_the_linear_oracle():
    """loss='linear' in the robust model is oracle/trf_lsmr.py: the same decisions, the same cameras."""
    case = bc.make_case("three")
    R, t, res = bc.oracle_solve("three")
    R2, t2, res2 = bro.bundle_adjust(case["points2d_px"], case["R_init"], case["tvec_init"], case["intr"], "linear", 1.0)
    assert (res2["nfev"], res2["status"], res2["lsmr_iters"]) == (res["nfev"], res["status"], res["lsmr_iters"])
    assert np.abs(R - R2).max() < 1e-12 and np.abs(t - t2).max() < 1e-10


# ---- the inputs of the kernel-level device test ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", brc.EVAL_CASES)
def test_eval_inputs_reach_both_sides_and_stay_away_from_the_clamp(name):
    case = bc.make_case(name)
    px, mask, obs_xy = brc.eval_input(name)
    assert int(mask.sum()) == brc.EVAL_PLANTED[name] and obs_xy.shape == (case["nobs"], 2)
    moved = np.linalg.norm(obs_xy - case["obs_xy"], axis=1)
    assert np.allclose(moved[mask], brc.EVAL_SHIFT, rtol=1e-12) and (moved[~mask] == 0).all()
    for x0 in bc.eval_points(name):
        r = eval_blocks(x0, case["ncam"], case["intr"], case["cam_idx"], case["pt_idx"], obs_xy)[0]
        for C in brc.EVAL_F_SCALES:
            z = (r / C) ** 2
            assert (z < 1).any() and (z > 1).any(), (name, C)
            assert (np.abs(z - 1) > 1e-9).all()                     # (huber's branch is not in doubt either)
            for loss in ("cauchy", "arctan"):
                brc.assert_away_from_the_clamp(name, loss, z)
                assert bro.row_scale(loss, r, C)[3].any(), "no clamped row: the clamp would go untested"
            assert bro.row_scale("huber", r, C)[3].any() and not bro.row_scale("soft_l1", r, C)[3].any()


# ---- the whole solves: decisions that do not hang on the last bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("key", brc.SOLVE_NAMES)
def test_whole_solve_decisions_do_not_hang_on_the_last_bits(key):
    want = brc.SOLVES[key]
    case, (px, _) = bc.make_case(want["case"]), brc.solve_input(key)
    R, t, res = brc.oracle_solve(key)
    decisions = (res["nfev"], res["status"], res["lsmr_iters"])
    assert decisions == (want["nfev"], want["status"], want["lsmr_iters"])
    sR = st = sc = 0.0
    for seed in (2000, 2001, 2002):
        rng = np.random.default_rng(seed)
        R2, t2, r2 = bro.bundle_adjust(px * (1 + 1e-15 * rng.normal(size=px.shape)), case["R_init"], case["tvec_init"], case["intr"], want["loss"], want["f_scale"])
        assert (r2["nfev"], r2["status"], r2["lsmr_iters"]) == decisions, seed
        sR, st, sc = max(sR, np.abs(R - R2).max()), max(st, np.abs(t - t2).max()), max(sc, abs(r2["cost"] - res["cost"]) / res["cost"])
    # the device starts from ITS triangulation, held to 1e-9 mm of the oracle's (tests/test_gpu_geometry.py): start points moved that far
    pts0 = og.triangulate_dlt_batched(px, og.projection_matrices(case["R_init"], case["tvec_init"], case["intr"]))
    for seed in (6000, 6001):
        rng = np.random.default_rng(seed)
        r2 = bro.bundle_adjust(px, case["R_init"], case["tvec_init"], case["intr"], want["loss"], want["f_scale"], pts0=pts0 + 1e-9 * rng.normal(size=pts0.shape))[2]
        assert (r2["nfev"], r2["status"], r2["lsmr_iters"]) == decisions, seed
    print("%s: nfev %d status %d lsmr %s spread_R %.2e spread_t %.2e spread_cost %.2e" % (key, *decisions, sR, st, sc))
    for got, name in ((sR, "spread_R"), (st, "spread_t"), (sc, "spread_cost")):   # the record is this measurement, rounded up
        assert want[name] / 100 <= got <= 2 * want[name], (name, got)


def test_the_solve_cases_cover_what_they_are_for():
    cases = {s["case"] for s in brc.SOLVES.values()}
    assert {"three", "mixed"} <= cases and len(brc.SOLVES) >= 3
    assert any(bc.CASES[s["case"]]["nobs"] >= 1024 for s in brc.SOLVES.values())       # two workgroups of the data-local LSMR form
    soft = [s for s in brc.SOLVES.values() if s["loss"] == "soft_l1"]
    assert any(s["fraction"] > 0 for s in soft) and len(soft) >= 4 and {s["case"] for s in soft} >= {"three", "mixed", "eight_1032"}
    # the other three losses: each solved with, to convergence, with outliers present; the stall -- rejected trials up to xtol -- at least once
    for loss in ("huber", "cauchy", "arctan"):
        assert any(s["loss"] == loss and s.get("kind") == "converging" and s["fraction"] > 0 and s["status"] == 2 for s in brc.SOLVES.values()), loss
    stalls = [s for s in brc.SOLVES.values() if s.get("kind") == "stall"]
    assert stalls and all(s["status"] == 4 and s["nfev"] - len(s["lsmr_iters"]) - 1 >= 10 for s in stalls)
    assert all(s["loss"] in brc.ROBUST for s in brc.SOLVES.values())
    # huber beyond z = 1 (its only branch that differs from the linear loss) is in some solve's start
    def rows_beyond_one(s):
        case, (px, _) = bc.make_case(s["case"]), brc.plant(s["case"], s["fraction"], s["shift"], s["seed"])
        pr = bro.problem(px, case["R_init"], case["tvec_init"], case["intr"])
        return int((np.abs(pr["evaluate"](pr["x0"], False)[0]) > s["f_scale"]).sum())
    assert any(s["loss"] == "huber" and s["status"] == 2 and rows_beyond_one(s) > 0 for s in brc.SOLVES.values())


# ---- the outcome test's input conditions, on the oracle alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(brc.OUTCOME))
def test_outcome_input_conditions(name):
    (px, mask), ora = brc.outcome_input(name), brc.outcome_oracle(name)
    assert int(mask.sum()) == max(1, int(round(0.05 * bc.CASES[name]["nobs"])))
    w = ora["robust"][2]["obs_weight"]
    low_planted, low_clean = float((w[mask] < 0.5).mean()), float((w[~mask] < 0.5).mean())
    print("%s: clean reprojection error: true %.3f linear %.3f robust %.3f (ratio %.2f); weight < 0.5: %.1f %% of the planted, %.2f %% of the clean"
          % (name, ora["true_err"], ora["linear_err"], ora["robust_err"], ora["robust_err"] / ora["linear_err"], 100 * low_planted, 100 * low_clean))
    assert ora["robust_err"] <= 0.8 * ora["linear_err"]
    assert low_planted >= 0.9
    if name == "three":
        # the two-view limit: three quarters of this case's points have two views, the partner of a planted outlier is
        # then as far from the point as the outlier, and the oracle itself weighs 4 % of the clean observations below 0.5 -- every one
        # of them on a point with a planted outlier.  The device test holds the 2 % bar on the other points' observations here.
        shares = brc.shares_a_point_with_a_planted_outlier(name, mask)
        assert 0.02 < low_clean < 0.06 and ((w < 0.5) <= shares).all()
        assert float((w[~mask & ~shares] < 0.5).mean()) <= 0.02
    else:
        assert low_clean <= 0.02


# ---- the C ABI's argument checks, before any device work -----------------------------------------------------------------------------------------
def test_argument_validation_without_gpu(native_lib):
    from deepfly3d_amd import _native
    from test_ba_host_pinned import PTR, problem

    assert native_lib.df3d_version() == _native.ABI_VERSION == 610          # entries were added, none changed
    assert _native.BA_LOSSES == bro.LOSSES
    P = ctypes.byref(problem())
    res, out = ctypes.c_double(), (ctypes.c_double * 6)()

    def calls(loss=1, C=2.0, p=P, ptr=PTR):
        return {
            "df3d_ba_eval_robust": lambda: native_lib.df3d_ba_eval_robust(p, ptr, loss, C, None, ptr, PTR, PTR, None, None),
            "df3d_ba_robust_cost": lambda: native_lib.df3d_ba_robust_cost(ptr, 8, loss, C, ctypes.byref(res), PTR, None),
            "df3d_ba_trf_linearize_robust": lambda: native_lib.df3d_ba_trf_linearize_robust(p, ptr, loss, C, None, PTR, PTR, PTR, None, PTR, PTR, PTR, PTR, 1, PTR, None),
            "df3d_ba_trf_trial_robust": lambda: native_lib.df3d_ba_trf_trial_robust(p, loss, C, 0.5, 0.5, ptr, *([PTR] * 12), out, None),
        }

    for what, kw, text in (("unknown loss", dict(loss=5), b"unknown loss"), ("negative loss", dict(loss=-1), b"unknown loss"),
                           ("f_scale 0", dict(C=0.0), b"f_scale"), ("f_scale negative", dict(C=-1.0), b"f_scale"),
                           ("f_scale inf", dict(C=float("inf")), b"f_scale"), ("f_scale nan", dict(C=float("nan")), b"f_scale"),
                           ("null pointer", dict(ptr=None), b"null")):
        for entry, call in calls(**kw).items():
            assert call() == _native.DF3D_EINVAL, (entry, what)
            err = native_lib.df3d_last_error()
            assert text in err and entry.encode() in err, (entry, what, err)
    for entry, call in calls(p=None).items():
        if entry != "df3d_ba_robust_cost":
            assert call() == _native.DF3D_EINVAL and b"null problem" in native_lib.df3d_last_error(), entry
    assert native_lib.df3d_ba_eval_robust(P, PTR, 1, 2.0, None, PTR, PTR, None, None, None) == _native.DF3D_EINVAL     # Jc without Jp
    assert b"together" in native_lib.df3d_last_error()


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------------
def test_cli_and_config_surface(capsys):
    import inspect

    from deepfly3d_amd import bundle_adjust as ba
    from deepfly3d_amd import cli, config
    from deepfly3d_amd.camera_network import CameraNetwork
    from deepfly3d_amd.core import Core

    assert config.BA_LOSS == "linear" and config.BA_F_SCALE == 4.0 and config.BA_LOSSES == bro.LOSSES
    args = cli.parse_cli_args(["/tmp/x"])
    assert args.ba_loss is None and args.ba_f_scale is None
    args = cli.parse_cli_args(["/tmp/x", "--ba-loss", "soft_l1", "--ba-f-scale", "2.5"])
    assert (args.ba_loss, args.ba_f_scale) == ("soft_l1", 2.5)
    assert cli.parse_cli_args(["/tmp/x", "--ba-loss", "arctan"]).ba_f_scale is None
    for argv in (["--ba-loss", "tukey"], ["--ba-f-scale", "2"], ["--ba-loss", "linear", "--ba-f-scale", "2"], ["--ba-loss", "huber", "--ba-f-scale", "0"],
                 ["--ba-loss", "huber", "--ba-f-scale", "nan"], ["--ba-loss", "huber", "--ba-f-scale", "inf"]):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(["/tmp/x"] + argv)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--ba-loss" in text and "--ba-f-scale" in text and "nobody has measured" in text.split("--ba-f-scale")[-1][:400]
    for fn, names in ((ba.solve_trf, ("loss", "f_scale")), (ba.bundle_adjust, ("loss", "f_scale")), (CameraNetwork.bundle_adjust, ("loss", "f_scale")),
                      (Core.calibrate_calc, ("loss", "f_scale"))):
        params = inspect.signature(fn).parameters
        assert all(n in params for n in names), fn
    assert inspect.signature(ba.solve_trf).parameters["loss"].default == "linear" and inspect.signature(Core.calibrate_calc).parameters["loss"].default is None
    assert inspect.signature(Core.calibration_outliers).parameters["threshold"].default == 0.5
    assert ba.loss_code("soft_l1", 2) == (1, 2.0) and ba.loss_code("linear", 1.0)[0] == 0
    for bad in (("tukey", 1.0), ("huber", 0.0), ("huber", float("nan")), ("huber", float("inf")), ("huber", -1.0)):
        with pytest.raises(ValueError):
            ba.loss_code(*bad)
