"""CPU checks of the pose-chain sweep's cases (tests/pose_chain_cases.py), on the oracles alone: every condition that
tests/test_gpu_pose_chain_sweep.py leans on holds BEFORE a kernel runs -- the planted values are where the case says, the lengths sit on
the sides of the route switch the case table names, an independent statement of the kernel's triangulation method agrees with the SVD
oracle a decade under the device's bar on every case, the Procrustes oracle's own spread under last-bit noise is two decades under the
device's bar, and the degenerate fits have the ranks the kernel's branches are meant to meet."""
import itertools

import numpy as np
import pytest

import pose_chain_cases as pc
from oracle import geometry as og
from oracle import postprocess as pp


# ---------------------------------------------------------------- re-layout ----------------------------------------------------------
def test_relayout_cases():
    assert len(set(pc.ORDERINGS)) == 5040 and all(sorted(o) == list(range(7)) for o in pc.ORDERINGS)
    p = pc.relayout_input(2)
    assert p.dtype == np.float32 and p.shape == (7, 2, 19, 2) and (p >= 0).all() and (p <= 1).all()
    for cam in range(7):
        assert set(p[cam, 0, [0, 7, 18], 1]) == set(p[cam, 1, [16, 4, 11], 1]) == {np.float32(0), np.float32(1), pc.BELOW_ONE}
    assert float(pc.BELOW_ONE) == 1 - 2.0**-24
    # un-flipping in float32 would show: most of the random columns have a 1 - col that float32 cannot hold
    col = p[..., 1]
    assert ((np.float32(1) - col).astype(np.float64) != 1 - col.astype(np.float64)).mean() > 0.25
    # the oracle un-flips ALL 38 joints of the three left cameras (1.0 where nothing is seen) and reads float32 widened
    out = og.relayout_19_to_38(p, pc.ORDERINGS[0])
    assert out.dtype == np.float64 and (out[4:, :, :19, 1] == 1.0).all() and (out[3] == 0).all()
    assert out[5, 0, 19 + 18, 1] == 2.0**-24 and out[5, 0, 19 + 7, 1] == 0.0 and out[5, 0, 19, 1] == 1.0
    # the edge lengths: totals below one block, exact multiples of it and one past
    rem = {T: (7 * T * 38) % 256 for T in pc.RELAYOUT_EDGE_T}
    assert 7 * 1 * 38 > 256 > 0 and rem[256] == 0 and rem[255] != 0 and rem[257] != 0 and rem[1] == 10


# ---------------------------------------------------------------- triangulation ------------------------------------------------------
def test_triangulation_cases_method_agrees_with_the_svd_oracle_below_the_bar():
    """The condition behind the 1e-9 mm bar: eigh of A^T A / trace against the SVD of A, on every subset of the sweep."""
    P, centre = pc.rig()
    px, X = pc.detections()
    assert P.shape == (8, 3, 4) and px.shape == (8, pc.TRI_POINTS, 1, 2)
    assert [len([s for s in pc.TRI_SUBSETS if len(s) == k]) for k in (2, 3, 8)] == [28, 56, 1] and len(pc.TRI_SUBSETS) == 85
    worst = {}
    for cams in pc.TRI_SUBSETS:
        sub = pc.only_cameras(px, cams)
        assert (og.visibility(sub).sum(axis=0) == len(cams)).all()
        ref = pc.tri_oracle(cams)
        assert np.abs(ref[:, 0] - X).max() < 5.0          # the oracle is near the true points: a solved problem, not a degenerate one
        e = np.abs(pc.triangulate_eigh(sub, P) - ref).max()
        if e >= worst.get(len(cams), (0.0, None))[0]:
            worst[len(cams)] = (e, cams)
    for k, (e, cams) in worst.items():
        print("triangulation, %d cameras: worst |eigh - SVD| %.2e mm at %s (condition %.0e, bar %.0e)" % (k, e, cams, pc.TRI_CONDITION, pc.TRI_BAR))
    assert max(e for e, _ in worst.values()) <= pc.TRI_CONDITION


def test_triangulation_visibility_rule_of_the_oracle():
    P, _ = pc.rig()
    px = pc.visibility_case()
    assert og.visibility(px).sum(axis=0)[:, 0].tolist() == [2, 0, 6, 1]
    ref = og.triangulate_dlt(px, P)
    assert (ref[0] != 0).all() and (ref[1] == 0).all() and (ref[3] == 0).all()
    assert np.array_equal(ref[2], og.triangulate_dlt(pc.only_cameras(px, range(2, 8)), P)[2])


# ---------------------------------------------------------------- medians ------------------------------------------------------------
def test_median_lengths_sit_where_the_case_table_says():
    long_route = [T * J >= pc.MED_LONG for T, J in pc.NORMALIZE_SHAPES]
    assert long_route == [False, True, True, True, True, False, True, True, True]
    assert [T * J for T, J in pc.NORMALIZE_SHAPES[5:]] == [65512, 65550, 65540, 65600]
    blocks = [-(-T * J // 4096) for T, J in pc.NORMALIZE_SHAPES]       # workgroups per column of the long route
    assert blocks[1:5] == [16, 17, 20, 21]
    assert pc.MED_LONG_WORK == 824
    assert [T * 19 >= pc.MED_LONG for T in pc.PROCRUSTES_SWITCH_T] == [False, True]
    assert all(n < pc.MED_LONG or n in (65536, 65537) for n in pc.COLUMN_MEDIAN_N)


@pytest.mark.parametrize("n", [2, 256, 257, 65536, 65537])
def test_median_columns_go_the_way_their_kind_says(n):
    key = lambda v: np.where(v.view(np.int64) < 0, ~v.view(np.uint64), v.view(np.uint64) | np.uint64(1 << 63))   # order_key of pose3d.hip
    c = {k: pc.median_column(k, n) for k in pc.COLUMN_KINDS}
    assert all(v.shape == (n,) and v.dtype == np.float64 for v in c.values())
    assert len(set(c["equal"])) == 1
    lo, hi = np.sort(c["halves"])[[(n - 1) // 2, n // 2]]
    if n % 2 == 0:
        assert (lo, hi) == (-1.25, 3.5) and (c["halves"] == 3.5).sum() == n // 2           # the middle ranks part at the sign bit
    assert len(set(key(c["low_byte"]) >> np.uint64(8))) == 1 and (n < 256 or len(set(c["low_byte"])) > 100)
    assert set(np.abs(c["signed_zeros"])) == {0.0} and len(set(np.signbit(c["signed_zeros"]))) == 2
    assert (n <= 3 or np.isinf(c["infs"]).any()) and np.isfinite(np.median(c["infs"])) and (n < 24 or len(set(c["infs"][np.isinf(c["infs"])])) == 2)
    assert (np.abs(c["denormals"]) < np.finfo(np.float64).tiny).all() and (c["denormals"] != 0).sum() >= n - 1
    assert (np.diff(c["sorted"]) > 0).all() and (np.diff(c["reversed"]) < 0).all()
    assert n < 256 or len(set(c["ties"])) < n // 2
    runs = pc.median_runs(n)
    assert len(runs) == 3 and all(r.shape == (n, 3) for r in runs)
    # the uint64 image orders like the doubles (-0.0 below +0.0, which numpy's median cannot tell apart: array_equal neither)
    v = c["infs"]
    assert np.array_equal(np.argsort(key(v), kind="stable"), np.argsort(v, kind="stable"))


# ---------------------------------------------------------------- Procrustes ---------------------------------------------------------
def test_procrustes_oracle_spread_under_last_bit_noise():
    """The condition behind the 1e-10 bar, over every draw of the sweep; and that the draws are what the case says."""
    rng = np.random.default_rng(1)
    spread, smin, dets = 0.0, np.inf, []
    for name, tmpl in pc.templates().items():
        assert tmpl.shape[1:] == (38, 3)
        for T in pc.PROCRUSTES_T:
            for draw in range(pc.PROCRUSTES_DRAWS):
                X = pc.moved_pose(T, draw)
                a = og.procrustes_separate(X, tmpl)
                b = og.procrustes_separate(X * (1 + 4 * pc.EPS * rng.uniform(-1, 1, size=X.shape)), tmpl)
                assert X.shape == (T, 38, 3) and np.isfinite(a).all()
                spread = max(spread, np.abs(a - b).max())
                for side in pc.SIDES:
                    sv = np.linalg.svd(pc.side_fit(X[:, side], tmpl[:, side])["G"])[1]
                    smin = min(smin, sv[2] / sv[0])
    for draw in range(6):
        Q, s, off = pc.rigid_motion(np.random.default_rng([97, 15, draw]), reflect=draw % 3 == 2)
        assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-14 and 0.1 <= s <= 10
        dets.append(round(np.linalg.det(Q)))
    assert dets == [1, 1, -1, 1, 1, -1]
    print("Procrustes oracle: spread %.2e over %d draws (condition %.0e, bar %.0e); smallest s_min / s_max %.2e (cut %.0e)"
          % (spread, 2 * len(pc.PROCRUSTES_T) * pc.PROCRUSTES_DRAWS, pc.PROCRUSTES_CONDITION, pc.PROCRUSTES_BAR, smin, pc.RANK_CUT))
    assert spread <= pc.PROCRUSTES_CONDITION
    assert smin > 1e6 * pc.RANK_CUT        # every draw is a full-rank fit, far from the kernel's weak branch


def test_procrustes_switch_sequences_are_full_rank():
    tmpl = pc.templates()["golden"]
    X = pc.long_pose(3450)
    assert X.shape == (3450, 38, 3) and np.array_equal(pc.long_pose(3449), X[:3449])
    for side in pc.SIDES:
        sv = np.linalg.svd(pc.side_fit(X[:, side], tmpl[:, side])["G"])[1]
        assert sv[2] > 1e6 * pc.RANK_CUT * sv[0]


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("case,null", [("coplanar", 1), ("collinear", 2)])
def test_degenerate_fits_have_the_stated_rank_and_a_unique_map_of_the_fit_joints(case, null, side):
    tmpl = pc.templates()["default"]
    X = pc.degenerate_pose(case, side)
    f = pc.side_fit(X[:, pc.SIDES[side]], tmpl[:, pc.SIDES[side]])
    assert np.isfinite(f["s"]) and f["s"] > 0
    U, sv, Vt = np.linalg.svd(f["G"])
    print("%s, side %d: singular values of G %s" % (case, side, sv))
    assert int((sv < pc.RANK_CUT * sv[0]).sum()) == null
    assert len({tuple(y) for y in f["Y"]}) == 4 - null       # three distinct median fit joints (a plane), two (a line)
    assert np.abs(Vt.T @ U.T - f["Tm"]).max() < 1e-14         # the restated SVD is the oracle's
    want = f["Y"] @ f["Tm"] + f["c"]
    for flips in itertools.product((1.0, -1.0), repeat=null):  # every sign choice of the null directions: the fit joints go to the same place
        sign = np.ones(3)
        sign[3 - null :] = flips
        Tm = Vt.T @ (U * sign).T
        c = f["X"].mean(0) - f["Y"].mean(0) @ Tm
        assert np.abs(Tm.T @ Tm - np.eye(3)).max() < 1e-14
        assert np.abs(f["Y"] @ Tm + c - want).max() < 1e-12
    assert np.isfinite(pc.oracle_procrustes(X, tmpl)).all()
    # the other side is an ordinary full-rank fit
    other = pc.side_fit(X[:, pc.SIDES[1 - side]], tmpl[:, pc.SIDES[1 - side]])
    assert np.linalg.svd(other["G"])[1][2] > 1e6 * pc.RANK_CUT


@pytest.mark.parametrize("side", [0, 1])
def test_a_lost_side_can_only_be_nan(side):
    """A side that is zero throughout, or whose legs 2 and 3 are: at least eight of its twelve median segment lengths are 0, the median scale
    ratio is infinite and the scaled, centred fit joints are NaN or infinite -- so is the matrix the oracle hands to its SVD, which numpy
    either refuses (LinAlgError) or answers with NaN, as any arithmetic SVD does.  The device test therefore expects NaN on that side and
    takes the other side from the oracle's run of the clean pose, which does not depend on this side."""
    tmpl = pc.templates()["default"]
    for X in (pc.zero_side_pose(side), pc.zero_legs_pose(side)):
        assert (X[:, pc.SIDES[1 - side]] == pc.golden_pose()[:, pc.SIDES[1 - side]]).all()
        f = pc.side_fit(X[:, pc.SIDES[side]], tmpl[:, pc.SIDES[side]])
        assert np.isinf(f["s"]) or np.isnan(f["s"])
        assert not np.isfinite(f["Y"]).any() and np.isnan(f["G"]).all() and f["Tm"] is None
        try:
            out = pc.oracle_procrustes(X, tmpl)
        except np.linalg.LinAlgError:     # "SVD did not converge": LAPACK's answer to a NaN matrix in this numpy
            continue
        assert np.isnan(out[:, pc.SIDES[side]]).all()
        assert np.array_equal(out[:, pc.SIDES[1 - side]], pc.oracle_procrustes(pc.golden_pose(), tmpl)[:, pc.SIDES[1 - side]])


# ---------------------------------------------------------------- One-Euro -----------------------------------------------------------
def test_oneeuro_cases():
    for T, nch in itertools.product(pc.ONEEURO_T, pc.ONEEURO_NCH):
        x = pc.oneeuro_input(T, nch)
        y = pp.oneeuro_filter(x)
        assert x.shape == y.shape == (T, nch) and np.array_equal(y[0], x[0]) and (T == 1 or not np.array_equal(y[1:], x[1:]))
    assert {n % 64 for n in pc.ONEEURO_NCH} == {1, 63, 0}
