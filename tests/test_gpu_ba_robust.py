"""-m gpu tests of the robust-loss bundle adjustment: df3d_ba_eval_robust, df3d_ba_robust_cost and the two fused
driver entries of csrc/ba.hip, solve_trf(loss=, f_scale=) and Core.calibrate_calc(loss=), against the float64 model of
tests/ba_robust_oracle.py on the planted-outlier inputs of tests/ba_robust_cases.py.  tests/test_ba_robust_host.py checks on the CPU every
condition relied on here (the oracle against scipy, the decisions' robustness, the outcome test's input conditions).  Every launch goes on
one side stream; every output buffer is filled with NaN in front of the call under test."""
import types

import numpy as np
import pytest
import torch

import ba_cases as bc
import ba_robust_cases as brc
import ba_robust_oracle as bro

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ULP = 64 * EPS          # scaled f, weights, scaled J: at most about six correctly rounded or 1-2 ulp operations past df3d_ba_eval's values


@pytest.fixture(scope="module")
def stream(native_lib, cuda):
    return torch.cuda.Stream(device=cuda)


@pytest.fixture(autouse=True)
def _on_the_side_stream(stream):
    with torch.cuda.stream(stream):
        yield
    stream.synchronize()


def _nan(n, cuda):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=cuda)


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _blocks(Jc, Jp, nobs):
    """The plane-major device layout as the oracle's (n, 2, 6) and (n, 2, 3)."""
    return Jc.cpu().numpy().reshape(2, 6, nobs).transpose(2, 0, 1), Jp.cpu().numpy().reshape(2, 3, nobs).transpose(2, 0, 1)


def _rel(got, want):
    """max |got - want| / |want| where want != 0; elements where want == 0 must be 0."""
    zero = want == 0
    assert np.array_equal(got[zero], want[zero])
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if (~zero).any() else 0.0


@pytest.fixture(scope="module", params=brc.EVAL_CASES)
def dev(request, native_lib, cuda, stream):
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, _Dev

    name = request.param
    case = bc.make_case(name)
    px, mask, obs_xy = brc.eval_input(name)
    with torch.cuda.stream(stream):
        prob = BAProblemDevice(px, case["intr"], cuda, min_views=case["min_views"])
        dv = _Dev(prob)
        stream.synchronize()
    assert (prob.nobs, prob.npts) == (case["nobs"], case["npts"]) and np.array_equal(prob.t["obs_xy"].cpu().numpy(), obs_xy)
    return types.SimpleNamespace(name=name, case=case, prob=prob, dv=dv)


def test_robust_eval_and_cost(dev, cuda):
    """Scaled f, weights and scaled Jacobian rows within 64 ulp of the oracle's on the device's own unscaled residuals and Jacobian, the
    set of clamped rows exactly, the cost within 1e-13, null outputs change nothing else, two runs bit-equal."""
    from deepfly3d_amd import _native

    prob, dv, nobs, m = dev.prob, dev.dv, dev.case["nobs"], dev.prob.m
    sqrt_eps = float(np.sqrt(EPS))      # 2^-26: a clamped row is the unscaled row times exactly this
    for which, x0 in enumerate(bc.eval_points(dev.name)):
        x = _up(x0, cuda)
        r, Jc, Jp = _nan(m, cuda), _nan(12 * nobs, cuda), _nan(6 * nobs, cuda)
        dv.eval(x, r, Jc, Jp)
        Jc0, Jp0 = _blocks(Jc, Jp, nobs)
        for loss in bro.LOSSES:
            code = _native.BA_LOSSES.index(loss)
            for C in brc.EVAL_F_SCALES:
                ft, f, w, Jcs, Jps = _nan(m, cuda), _nan(m, cuda), _nan(m, cuda), _nan(12 * nobs, cuda), _nan(6 * nobs, cuda)
                dv.eval_robust(x, code, C, f, Jcs, Jps, f_true=ft, w=w)
                f_true = ft.cpu().numpy()
                e_true = float(np.abs(f_true - r.cpu().numpy()).max() / np.abs(f_true).max())
                assert e_true <= 8 * EPS, (dev.name, loss, C, e_true)          # the unscaled residuals are df3d_ba_eval's statements again
                z, _, s, clamped = bro.row_scale(loss, f_true, C)
                assert (z < 1).any() and (z > 1).any(), "the input has to have residuals on both sides of z = 1"
                if loss in ("cauchy", "arctan"):
                    brc.assert_away_from_the_clamp(dev.name, loss, z)
                want_f, want_Jc, want_Jp, want_w, _ = bro.scale_rows(loss, C, f_true, Jc0, Jp0)
                got_Jc, got_Jp = _blocks(Jcs, Jps, nobs)
                e = dict(f=_rel(f.cpu().numpy(), want_f), w=_rel(w.cpu().numpy(), want_w), Jc=_rel(got_Jc, want_Jc), Jp=_rel(got_Jp, want_Jp))
                print("%s[%d] %s C=%g: true f vs df3d_ba_eval %.1e;  vs oracle (bar 64 ulp = %.1e): %s;  %d of %d rows clamped"
                      % (dev.name, which, loss, C, e_true, ULP, "  ".join("%s %.1e" % kv for kv in e.items()), int(clamped.sum()), m))
                assert max(e.values()) <= ULP, (dev.name, loss, C, e)
                # the clamped rows, exactly: such a row of Jp (never all zero: dpi R) is the unscaled row times 2^-26 to the bit
                got_clamped = (got_Jp == Jp0 * sqrt_eps).all(axis=2).reshape(-1)
                assert np.array_equal(got_clamped, clamped), (dev.name, loss, C)
                # null outputs: nothing else changes
                f2 = _nan(m, cuda)
                dv.eval_robust(x, code, C, f2)
                assert torch.equal(f2, f)
                f3, Jc3, Jp3 = _nan(m, cuda), _nan(12 * nobs, cuda), _nan(6 * nobs, cuda)
                dv.eval_robust(x, code, C, f3, Jc3, Jp3)
                assert torch.equal(f3, f) and torch.equal(Jc3, Jcs) and torch.equal(Jp3, Jps)
                # the cost of the unscaled residuals
                cost = dv.robust_cost(ft, code, C)
                want = bro.robust_cost(loss, f_true, C)
                assert abs(cost - want) <= 1e-13 * want, (dev.name, loss, C, cost, want)
                assert dv.robust_cost(ft, code, C) == cost                      # a second run: the same bits


def test_linear_is_untouched(native_lib, cuda):
    """loss='linear' spelled out, and no loss argument at all: the same x, nfev and LSMR counts to the bit, and no new key."""
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, bundle_adjust, solve_trf

    for name in ("three", "eight_1032"):
        case = bc.make_case(name)
        prob = BAProblemDevice(case["points2d_px"], case["intr"], cuda)
        x0 = _up(case["x0"], cuda)
        a, b = solve_trf(prob, x0), solve_trf(prob, x0, loss="linear", f_scale=3.0)
        assert torch.equal(a["x"], b["x"]) and (a["nfev"], a["status"], a["lsmr_iters"], a["cost"]) == (b["nfev"], b["status"], b["lsmr_iters"], b["cost"])
        assert set(a) == set(b) and "weights" not in a and "loss" not in a
        Ra, ta, ia = bundle_adjust(case["points2d_px"], case["R_init"], case["tvec_init"], case["intr"], device=cuda, return_info=True)
        Rb, tb, ib = bundle_adjust(case["points2d_px"], case["R_init"], case["tvec_init"], case["intr"], device=cuda, return_info=True, loss="linear")
        want = bc.SOLVES[name]
        assert np.array_equal(Ra, Rb) and np.array_equal(ta, tb) and torch.equal(ia["x"], ib["x"])
        assert (ia["nfev"], ia["status"], ia["lsmr_iters"]) == (ib["nfev"], ib["status"], ib["lsmr_iters"]) == (want["nfev"], want["status"], want["lsmr_iters"])
        assert set(ia) == set(ib) and "obs_weight" not in ia


def _assert_the_stall(key, form, want, case, px, info, res, cuda):
    """The stalled solve is there for its run of rejected trials: nfev - len(lsmr_iters) - 1 of them happened, and the weights it
    returns are those of the point it stalled at, within 64 ulp.
    The reference for the weights is the oracle's rho' of the device's own unscaled residuals at the device's final x (one more
    df3d_ba_eval_robust there), as test_robust_eval_and_cost takes it.  The oracle's own final weights cannot serve at that bar, nor can
    the oracle's residuals at the device's x (both printed beside it): a residual is the difference of two pixel coordinates of some
    500 px, so two correct evaluations differ by EPS x 500 px, 100 EPS of a 5 px residual, before a weight is formed (measured: 3.3e-14
    for huber, 2.3e-14 for cauchy); and the device starts from its own triangulation, held to 1e-9 mm of the oracle's
    (tests/test_gpu_geometry.py), where a start moved by 1e-14 mm moves this solve's final weights by 61 x 64 ulp (measured on the
    oracle: DESIGN.md section 26, "Sweep")."""
    from deepfly3d_amd import _native
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, _Dev

    rejected = info["nfev"] - len(info["lsmr_iters"]) - 1
    assert rejected == want["nfev"] - len(want["lsmr_iters"]) - 1 >= 10, (key, form, rejected)
    loss, C = want["loss"], want["f_scale"]
    prob = BAProblemDevice(px, case["intr"], cuda)
    f, ft, wd = _nan(prob.m, cuda), _nan(prob.m, cuda), _nan(prob.m, cuda)
    _Dev(prob).eval_robust(info["x"], _native.BA_LOSSES.index(loss), C, f, f_true=ft, w=wd)
    want_w = bro.weight(loss, (ft.cpu().numpy() / C) ** 2).reshape(-1, 2).min(axis=1)
    f_host = bro.problem(px, case["R_init"], case["tvec_init"], case["intr"])["evaluate"](info["x"].cpu().numpy(), False)[0]
    w = info["weights"].cpu().numpy()
    e_w = _rel(w, want_w)
    print("%s form %s: %d rejected trials; weights vs the oracle's rho' of the device's residuals at its x %.2e (bar 64 ulp = %.1e); of the oracle's "
          "residuals at that x %.2e; vs the oracle's own final weights %.2e"
          % (key, form, rejected, e_w, ULP, _rel(w, bro.weight(loss, (f_host / C) ** 2).reshape(-1, 2).min(axis=1)), _rel(w, res["obs_weight"])))
    assert (want_w < 0.5).any() and (want_w > 0.9).any()          # (weights that say something)
    assert np.array_equal(w, wd.view(-1, 2).min(dim=1).values.cpu().numpy())     # what the solve kept through its rejections: the last linearisation's
    assert e_w <= ULP, (key, form, e_w)


@pytest.mark.parametrize("key", brc.SOLVE_NAMES)
def test_whole_solve(native_lib, cuda, monkeypatch, key):
    """nfev, status and LSMR counts are the oracle's; R, t and the cost within 100 x the oracle's own spread; the two back ends take the
    same decisions and give the same bits; every LSMR form is accepted."""
    from deepfly3d_amd.bundle_adjust import bundle_adjust

    want = brc.SOLVES[key]
    case, (px, _) = bc.make_case(want["case"]), brc.solve_input(key)
    Ro, to, res = brc.oracle_solve(key)
    assert (res["nfev"], res["status"], res["lsmr_iters"]) == (want["nfev"], want["status"], want["lsmr_iters"])
    bar_R, bar_t, bar_c = max(100 * want["spread_R"], 1e-12), max(100 * want["spread_t"], 1e-12), max(100 * want["spread_cost"], 1e-13)
    for form in ("0", "2", "1", "11"):
        monkeypatch.setenv("DF3D_LSMR_KERNELS", form)
        got = []
        for host in (("1", "0") if form in ("0", "2") else ("0",)):
            monkeypatch.setenv("DF3D_TRF_HOST_SCALARS", host)
            R, t, info = bundle_adjust(px, case["R_init"], case["tvec_init"], case["intr"], device=cuda, return_info=True, loss=want["loss"], f_scale=want["f_scale"])
            got.append((R, t, info["cost"], info["nfev"], info["njev"], info["status"], info["lsmr_iters"], info["optimality"], info["lsmr_fallbacks"],
                        info["obs_weight"].tobytes()))
        R, t, cost = got[0][:3]
        e_c = abs(cost - res["cost"]) / res["cost"]
        print("%s form %s: nfev %d status %d lsmr %s  |R - oracle| %.2e (bar %.1e)  |t - oracle| %.2e (bar %.1e)  cost %.2e (bar %.1e)"
              % (key, form, got[0][3], got[0][5], got[0][6], np.abs(R - Ro).max(), bar_R, np.abs(t - to).max(), bar_t, e_c, bar_c))
        if len(got) == 2:
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2:] == got[1][2:], form   # bit for bit
        assert (got[0][3], got[0][5], got[0][6]) == (res["nfev"], res["status"], res["lsmr_iters"]), form
        assert got[0][8] == 0
        assert np.abs(R - Ro).max() <= bar_R and np.abs(t - to).max() <= bar_t and e_c <= bar_c, form
        assert (info["loss"], info["f_scale"]) == (want["loss"], want["f_scale"])
        if want.get("kind") == "stall":
            _assert_the_stall(key, form, want, case, px, info, res, cuda)


@pytest.mark.parametrize("name", tuple(brc.OUTCOME))
def test_outcome(native_lib, cuda, name):
    """5 % outliers at 40 px, soft_l1, f_scale 2: the device's cameras re-project the CLEAN detections as well as the oracle's robust
    solve does (a weighting that is wrong or not applied lands at the linear value, 1.25 x or more above), and the weights point at the
    planted outliers."""
    from deepfly3d_amd.bundle_adjust import bundle_adjust

    case, (px, mask), ora = bc.make_case(name), brc.outcome_input(name), brc.outcome_oracle(name)
    assert ora["robust_err"] <= 0.8 * ora["linear_err"]
    R, t, info = bundle_adjust(px, case["R_init"], case["tvec_init"], case["intr"], device=cuda, return_info=True, loss=brc.OUTCOME_LOSS, f_scale=brc.OUTCOME_F_SCALE)
    err = bro.clean_reprojection_error(case["points2d_px"], R, t, case["intr"])
    w = info["weights"].cpu().numpy()
    clean = ~mask
    if name == "three":
        # three quarters of this case's points are seen by two cameras: the partner of a planted outlier there is as far from the point
        # as the outlier is (the two-view limit), and the ORACLE weighs 4.0 % of all clean observations below 0.5,
        # every one of them on a point with a planted outlier (tests/test_ba_robust_host.py asserts both).  So the 2 % bar is held on the
        # clean observations of the other points here, and in full on the two cases where every point has seven or eight views to judge by
        clean &= ~brc.shares_a_point_with_a_planted_outlier(name, mask)
    low_planted, low_clean = float((w[mask] < 0.5).mean()), float((w[clean] < 0.5).mean())
    print("%s: clean reprojection error: true cameras %.3f, oracle linear %.3f, oracle robust %.3f, device robust %.3f (bar %.3f); weight < 0.5: %.1f %% of the "
          "planted, %.2f %% of the clean; nfev %d" % (name, ora["true_err"], ora["linear_err"], ora["robust_err"], err, 1.05 * ora["robust_err"],
                                                     100 * low_planted, 100 * low_clean, info["nfev"]))
    assert err <= 1.05 * ora["robust_err"]
    assert low_planted >= 0.9 and low_clean <= 0.02
    # the weights on the detections' grid: NaN exactly where there is no observation, the solver's weights elsewhere
    grid = info["obs_weight"]
    seen = (px[..., 0] != 0) & (px[..., 1] != 0)
    assert grid.shape == px.shape[:3] and np.array_equal(np.isnan(grid), ~seen)
    order = brc.observation_order(px)
    assert np.array_equal(grid[order[:, 2], order[:, 0], order[:, 1]], w)



def _golden_core(tmp_path, golden_dir, name):
    import os

    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder = tmp_path / name
    folder.mkdir()
    for f in os.listdir(os.path.join(golden_dir, "images")):
        os.symlink(os.path.join(golden_dir, "images", f), folder / f)
    g2 = np.load(f"{golden_dir}/golden_2d.npz")
    core = Core(str(folder), str(tmp_path / (name + "_df3d")), num_images_max=0, camera_ordering=[0, 1, 2, 3, 4, 5, 6])
    core.num_images = 15
    core.points2d = g2["points2d"]
    core.conf = g2["heatmap_confidence"]
    return core


def test_core_surface(native_lib, cuda, tmp_path, golden_dir):
    """Core.calibrate_calc(loss='soft_l1') on the golden sample: the three keys behind every other key with the stated shapes, ba_weight NaN
    exactly where the observation table has no entry, calibration_outliers() = ba_weight below the threshold; a linear calibration
    writes the bytes it always wrote."""
    import pickle

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    saved = {}
    for name, kw in (("plain", {}), ("linear", dict(loss="linear", f_scale=2.0)), ("robust", dict(loss="soft_l1"))):
        core = _golden_core(tmp_path, golden_dir, name)
        core.calibrate_calc(0, 100, **kw)
        core.save()
        with open(core.save_path, "rb") as f:
            saved[name] = f.read()
        if name != "robust":
            with pytest.raises(RuntimeError, match="robust calibration"):
                core.calibration_outliers()
    assert saved["plain"] == saved["linear"]
    plain, robust = pickle.loads(saved["plain"]), pickle.loads(saved["robust"])
    assert [str(k) for k in plain.keys()] == list(g3["key_order"])
    assert [str(k) for k in robust.keys()] == list(g3["key_order"]) + ["ba_weight", "ba_counts", "ba_params"]
    w, counts, params = robust["ba_weight"], robust["ba_counts"], robust["ba_params"]
    px = core.camNet.points2d
    assert w.shape == (7, 15, 38) == px.shape[:3] and w.dtype == np.float64 and counts.shape == (7, 3)
    seen = (px[..., 0] != 0) & (px[..., 1] != 0)
    in_table = seen & (seen.sum(axis=0) >= 2)[None]
    assert np.array_equal(np.isnan(w), ~in_table)
    assert (w[in_table] > 0).all() and (w[in_table] <= 1).all()
    from deepfly3d_amd import config as cfg

    assert params["loss"] == "soft_l1" and params["f_scale"] == cfg.BA_F_SCALE == 4.0 and cfg.BA_LOSS == "linear"
    assert np.array_equal(counts[:, 0], in_table.sum(axis=(1, 2)))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(counts[:, 1], (w < 0.5).sum(axis=(1, 2)))
        for thr in (0.5, 0.9):
            assert core.calibration_outliers(thr) == [tuple(int(v) for v in idx) for idx in np.argwhere(w < thr)]
    with np.errstate(invalid="ignore", divide="ignore"):   # (a camera without an observation in the table -- the sample has one -- has no mean)
        assert np.allclose(counts[:, 2], np.nansum(w, axis=(1, 2)) / counts[:, 0], rtol=1e-15, equal_nan=True)
    assert np.array_equal(np.isnan(counts[:, 2]), counts[:, 0] == 0)
    with pytest.raises(ValueError):
        core.calibration_outliers(0.0)
    with pytest.raises(ValueError):
        core.calibrate_calc(0, 100, loss="tukey")
    with pytest.raises(ValueError):
        core.calibrate_calc(0, 100, loss="soft_l1", f_scale=0.0)
