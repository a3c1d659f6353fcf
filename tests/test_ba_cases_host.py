"""CPU checks of the bundle-adjustment sweep's cases (tests/ba_cases.py), on the oracle alone: every condition that
tests/test_gpu_ba_sweep.py relies on holds BEFORE a kernel runs -- the tables have the stated counts, the data-local form's partition cuts
the ranges the case table names, the oracle's stop decisions do not hang on the last bit of its input, and its own error at small rotations
leaves a decade under the device's bar."""
import numpy as np
import pytest

import ba_cases as bc
from oracle import geometry as og
from oracle import trf_lsmr as ot

# ---- csrc/ba_lsmr.hip restated: lsmr_local_partition_kernel and local_workgroups_for.  If LT, LK, LMAXG or the partition there change, this
# restatement and the expectations below change with them: they pin what the cases are meant to reach.
LT, LOBS, LMAXG = 512, 1024, 128


def local_workgroups_for(nobs):
    return (nobs + (LOBS - 8) - 1) // (LOBS - 8)


def local_partition(pt_start, nobs, gmax):
    """wg_obs[0 .. gmax]: greedy ranges of whole points, at most LOBS observations and LT points each."""
    npts, start, q, wg_obs = len(pt_start) - 1, 0, 0, [0]
    for _ in range(gmax):
        if start < nobs:
            hi = min(npts, q + LT)
            q = max(k for k in range(q, hi + 1) if pt_start[k] <= start + LOBS)
            start = int(pt_start[q])
        wg_obs.append(start)
    return wg_obs


def _tables(name):
    case = bc.make_case(name)
    counts = np.bincount(case["pt_idx"], minlength=case["npts"])
    return case, counts, np.concatenate([[0], np.cumsum(counts)])


# what the partition gives per case: G, observations per range, point owners per range
RANGES = {
    "tiny": (1, [2], [1]),
    "one_cam": (1, [300], [300]),
    "eight_1016": (1, [1016], [127]),
    "eight_1024": (2, [1024, 0], [128, 0]),                # a range of exactly LOBS observations, an empty second workgroup
    "eight_1032": (2, [1024, 8], [128, 1]),
    "pairs_512": (2, [1024, 0], [512, 0]),                 # exactly LT owners
    "pairs_513": (2, [1024, 2], [512, 1]),
    "max_fit": (128, [1024] * 127 + [0], [128] * 127 + [0]),
}


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_tables_have_the_stated_counts(name):
    case, counts, pt_start = _tables(name)
    spec, vis = bc.CASES[name], case["vis"]
    cam_idx, pt_idx, obs_xy, slot = og.build_observations(case["points2d_px"], min_views=case["min_views"])
    assert cam_idx.size == case["nobs"] == int(vis.sum()) == spec["nobs"]
    assert int((slot >= 0).sum()) == case["npts"] == spec["npts"]
    assert np.array_equal(np.bincount(cam_idx, minlength=case["ncam"]), vis.sum(axis=0))   # per camera
    assert np.array_equal(counts, vis.sum(axis=1))                                          # views per point
    assert np.array_equal(pt_idx, np.repeat(np.arange(case["npts"]), counts))               # a point's observations are consecutive
    assert (case["m"], case["n"]) == (2 * case["nobs"], 6 * case["ncam"] + 3 * case["npts"])
    if name == "tiny":
        assert (case["m"], case["n"]) == (4, 15)
    if name == "one_cam":
        assert (counts == 1).all() and case["ncam"] == 1
    if name.startswith("pairs"):
        assert (counts == 2).all() and len({tuple(v) for v in vis}) == 21
    if name == "mixed":
        assert set(counts) == set(range(2, 8)) and 7000 < case["nobs"] < 8000
    if name == "edge_cams":
        per_cam = vis.sum(axis=0)
        assert per_cam[0] == 0 and per_cam[6] == 0 and per_cam[3] == 5 and (per_cam[[1, 2, 4, 5]] > 32).all()   # 5 < NCHUNK = 32 chunks
    if name in ("three", "small_rot"):
        assert np.array_equal(case["points2d_px"], bc.make_case("three")["points2d_px"]) and (counts >= 2).all()


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_partition_reaches_the_ranges_the_case_is_for(name):
    case, counts, pt_start = _tables(name)
    nobs, G = case["nobs"], local_workgroups_for(case["nobs"])
    if name == "over_fit":
        assert G == 129 and G > LMAXG                       # the data-local form refuses
        return
    assert G <= LMAXG
    wg = local_partition(pt_start, nobs, G)
    assert wg[-1] == nobs, "the ranges do not cover the observations: the form would refuse this case"
    sizes = np.diff(wg)
    owners = np.array([np.searchsorted(pt_start, b) - np.searchsorted(pt_start, a) for a, b in zip(wg[:-1], wg[1:])])
    assert (sizes <= LOBS).all() and (owners <= LT).all() and np.isin(wg, pt_start).all()   # whole points, within the kernel's layout
    if name in RANGES:
        assert (G, list(sizes), list(owners)) == RANGES[name]
    if name in ("three", "small_rot"):
        assert G == 1 and list(sizes) == [nobs]             # one range, smaller than LOBS - 8
    if name == "mixed":
        assert G == 8 and (sizes > 0).all() and len(set(sizes)) > 2                              # irregular cuts, no empty workgroup
        for a, b in zip(wg[:-1], wg[1:]):
            assert set(case["cam_idx"][a:b]) == set(range(7))                                    # every camera's list is spread over every range
    if name == "edge_cams":
        assert G == 2 and (sizes > 0).all()


# (istop, itn) of oracle.trf_lsmr.lsmr at the case's x0, damping 0.37 -- quoted here so that a change of a seed shows up
LSMR_STOPS = {"tiny": (2, 4), "one_cam": (2, 9), "three": (2, 22), "eight_1016": (2, 18), "eight_1024": (2, 18), "eight_1032": (2, 18), "pairs_512": (2, 26),
              "pairs_513": (2, 25), "mixed": (2, 22), "edge_cams": (2, 23), "max_fit": (2, 14), "over_fit": (2, 15), "small_rot": (2, 25)}


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_lsmr_stop_decision_does_not_hang_on_the_last_bits(name):
    case, r = bc.make_case(name), bc.oracle_blocks(name)[0]
    ref = bc.oracle_lsmr(name)
    rng = np.random.default_rng(1000)
    again = bc.oracle_lsmr(name, None, r * (1 + 1e-13 * rng.normal(size=r.size)))
    assert ref[1:3] == again[1:3] == LSMR_STOPS[name], (ref[1:3], again[1:3])
    maxiter = min(case["m"], case["n"])
    if name == "tiny":
        assert maxiter == 4            # capped on purpose: the run may use all of min(m, n)
    else:
        assert ref[2] < maxiter and ref[1] in (1, 2)


@pytest.mark.parametrize("name", ("tiny", "eight_1024", "mixed"))
def test_capped_lsmr_runs_are_capped(name):
    """The runs with maxiter 1, 15, 16, 17 of the device test end at maxiter (istop 7), so they compare iterates, not a converged solution."""
    case = bc.make_case(name)
    for maxiter in sorted({min(k, case["m"], case["n"]) for k in (1, 15, 16, 17)}):
        ref = bc.oracle_lsmr(name, maxiter)
        assert ref[2] == maxiter and (ref[1] == 7 or (name == "tiny" and maxiter == 4)), (maxiter, ref[1:3])


def _eval_blocks_longdouble(x, ncam, intr, cam_idx, pt_idx, obs_xy):
    """oracle.trf_lsmr.eval_blocks (and oracle.geometry.matrix_from_rotvec), formula for formula, in np.longdouble."""
    ld = np.longdouble
    x, intr, obs_xy = x.astype(ld), intr.astype(ld), obs_xy.astype(ld)
    cams, pts = x[: ncam * 6].reshape(ncam, 6), x[ncam * 6 :].reshape(-1, 3)
    eye = np.eye(3, dtype=ld)

    def skew(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=ld)

    Rs, Ms = [], []
    for c in range(ncam):
        r = cams[c, :3]
        th2 = r @ r
        th = np.sqrt(th2)
        if th < ld(1e-12):
            R = eye + skew(r)
        else:
            K = skew(r / th)
            R = eye + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        M = eye if th2 < ld(1e-24) else (np.outer(r, r) + (R.T - eye) @ skew(r)) / th2
        Rs.append(R)
        Ms.append(M)
    R, M, X = np.stack(Rs)[cam_idx], np.stack(Ms)[cam_idx], pts[pt_idx]
    Xc = np.einsum("nij,nj->ni", R, X) + cams[cam_idx, 3:]
    fx, fy, cx, cy = intr[cam_idx, 0, 0], intr[cam_idx, 1, 1], intr[cam_idx, 0, 2], intr[cam_idx, 1, 2]
    iz = 1 / Xc[:, 2]
    res = np.stack([fx * Xc[:, 0] * iz + cx - obs_xy[:, 0], fy * Xc[:, 1] * iz + cy - obs_xy[:, 1]], axis=1).ravel()
    n = cam_idx.size
    dpi = np.zeros((n, 2, 3), dtype=ld)
    dpi[:, 0, 0], dpi[:, 0, 2] = fx * iz, -fx * Xc[:, 0] * iz * iz
    dpi[:, 1, 1], dpi[:, 1, 2] = fy * iz, -fy * Xc[:, 1] * iz * iz
    Xx = np.zeros((n, 3, 3), dtype=ld)
    Xx[:, 0, 1], Xx[:, 0, 2] = -X[:, 2], X[:, 1]
    Xx[:, 1, 0], Xx[:, 1, 2] = X[:, 2], -X[:, 0]
    Xx[:, 2, 0], Xx[:, 2, 1] = -X[:, 1], X[:, 0]
    dXc = -np.einsum("nij,njk,nkl->nil", R, Xx, M)
    return res, np.concatenate([np.einsum("nij,njk->nik", dpi, dXc), dpi], axis=2), np.einsum("nij,njk->nik", dpi, R)


# measured error of the float64 oracle's Jc against the 80-bit evaluation, relative to max |Jc|:
#   small_rot vector 0 (|r| = 0, 1e-13, 1e-8):      see SMALL_ROT_MEASURED[0]: the 1e-8 camera's cancellation in M
#   small_rot vector 1 (|r| = 2e-12, 1e-6, pi-1e-6): see SMALL_ROT_MEASURED[1]
SMALL_ROT_MEASURED = (4.2e-9, 7.5e-11)


@pytest.mark.parametrize("which", (0, 1))
def test_oracle_error_at_small_rotations_is_a_decade_under_the_device_bar(which):
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is not the 80-bit extended format here: nothing more precise than the oracle to compare it with")
    case, x = bc.make_case("small_rot"), bc.small_rot_x0(which)
    norms = np.linalg.norm(x[:18].reshape(3, 6)[:, :3], axis=1)
    assert np.allclose(norms, bc.SMALL_ROT_NORMS[which], rtol=1e-12, atol=0) and (which == 1 or norms[0] == 0.0)
    r, Jc, Jp = ot.eval_blocks(x, 3, case["intr"], case["cam_idx"], case["pt_idx"], case["obs_xy"])
    rl, Jcl, Jpl = _eval_blocks_longdouble(x, 3, case["intr"], case["cam_idx"], case["pt_idx"], case["obs_xy"])
    e_r = float(np.abs(r - rl).max())
    e_Jc = float(np.abs(Jc - Jcl).max() / np.abs(Jcl).max())
    e_Jp = float(np.abs(Jp - Jpl).max() / np.abs(Jpl).max())
    print("small_rot %d: oracle vs longdouble: r %.2e px, Jc %.2e, Jp %.2e (relative to the block's largest entry)" % (which, e_r, e_Jc, e_Jp))
    assert e_Jc < 1e-8          # the device's bar for Jc is 1e-7: a decade over the oracle's own error
    assert e_Jc < 3 * SMALL_ROT_MEASURED[which]
    assert e_r < 1e-10 and e_Jp < 1e-10   # a decade under the device's 1e-9 bars
    if which == 0:              # cameras 0 and 1 take the first-order branch on both sides: no cancellation there
        for c in (0, 1):
            sel = case["cam_idx"] == c
            assert np.abs(Jc[sel] - Jcl[sel]).max() < 1e-13 * np.abs(Jcl).max()


@pytest.mark.parametrize("name", bc.SOLVE_CASES)
def test_whole_solve_decisions_do_not_hang_on_the_last_bits(name):
    case = bc.make_case(name)
    R, t, res = bc.oracle_solve(name)
    want = bc.SOLVES[name]
    assert (res["nfev"], res["status"], res["lsmr_iters"]) == (want["nfev"], want["status"], want["lsmr_iters"])
    spread_R = spread_t = 0.0
    for seed in (2000, 2001, 2002):
        rng = np.random.default_rng(seed)
        px = case["points2d_px"] * (1 + 1e-15 * rng.normal(size=case["points2d_px"].shape))
        R2, t2, res2 = ot.bundle_adjust(px, case["R_init"], case["tvec_init"], case["intr"], return_info=True)
        assert (res2["nfev"], res2["status"], res2["lsmr_iters"]) == (res["nfev"], res["status"], res["lsmr_iters"]), seed
        spread_R, spread_t = max(spread_R, np.abs(R - R2).max()), max(spread_t, np.abs(t - t2).max())
    # The device starts from ITS triangulation, which is held to 1e-9 mm of the oracle's (tests/test_gpu_geometry.py), not to the last bit.
    # Detections moved by a relative 3e-10 (1.5e-7 px, which moves the triangulated start points by about 1e-9 mm) must leave the decisions
    # alone too; the spread is not taken from these runs.
    for seed in (6000, 6001):
        rng = np.random.default_rng(seed)
        px = case["points2d_px"] * (1 + 3e-10 * rng.normal(size=case["points2d_px"].shape))
        res2 = ot.bundle_adjust(px, case["R_init"], case["tvec_init"], case["intr"], return_info=True)[2]
        assert (res2["nfev"], res2["status"], res2["lsmr_iters"]) == (res["nfev"], res["status"], res["lsmr_iters"]), seed
    print("%s: nfev %d status %d lsmr %s spread_R %.2e spread_t %.2e" % (name, res["nfev"], res["status"], res["lsmr_iters"], spread_R, spread_t))
    # the recorded spreads are this measurement, rounded up: the device's bars (100 x) are derived from the record
    assert spread_R <= 2 * want["spread_R"] and spread_t <= 2 * want["spread_t"]
    assert spread_R >= want["spread_R"] / 100 and spread_t >= want["spread_t"] / 100
