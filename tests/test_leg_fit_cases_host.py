"""CPU certification of tests/leg_fit_cases.py on the float64 oracle alone ("swept"): every family does what
it is there for -- pivot failures, rejections on cost, lambda climbing and coming back to 0, both statuses at the iteration limit,
the overflow stall, the ties and thresholds that take the branch they name, waves of mixed exit passes -- and the oracle's two
arithmetic paths agree as closely as leg_fit_cases.MEASURED says, which the bars of tests/test_gpu_leg_fit_sweep.py are built from.
The oracle's trace only listens."""
import numpy as np
import pytest

import leg_fit_cases as lc
import leg_fit_oracle as lo

NAMES = list(lc.families())
DEFAULT = [n for n in NAMES if lc.families()[n].max_iter == lo.MAX_ITER and n != "tie_step"]


def _records(f):
    return [r for row in f.traces for tr in row for r in tr]


def _rejections_then_acceptance(tr):
    """The longest run of rejected trials that an acceptance ends."""
    best = run = 0
    for r in tr:
        if r[2]:
            best, run = max(best, run), 0
        else:
            run += 1
    return best


def _returns_to_zero(tr):
    lams = [r[0] for r in tr]
    return any(a > 0.0 and b == 0.0 for a, b in zip(lams, lams[1:]))


def _highest_index_basis(d, basis_variant=False):
    """tangent_basis with the ties of the smallest component going to the HIGHEST index: what the model is not."""
    a = np.abs(d)
    e = np.zeros(3)
    e[2 - int(np.argmin(a[::-1]))] = 1.0
    b1 = np.cross(d, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return np.stack([b1, np.cross(d, b1)], axis=1)


# ------------------------------------------------------------------------------------------------------------------ the trace
def test_trace_changes_no_bits():
    n = 0
    for name in ("noisy", "stalled", "edges", "tie_step", "limited_3", "mixed_free"):
        fam = lc.families()[name]
        for t in range(0, len(fam.X), 5):
            for leg in range(6):
                P, a = fam.X[t, lo.leg_joints(leg)], None if fam.A is None else fam.A[leg]
                for variant in (False, True):
                    trace = []
                    with np.errstate(all="ignore"):
                        plain = lo.fit_leg(P, fam.L[leg], a, fam.max_iter, variant)
                        traced = lo.fit_leg(P, fam.L[leg], a, fam.max_iter, variant, trace=trace)
                    assert plain[0].tobytes() == traced[0].tobytes() and np.float64(plain[1]).tobytes() == np.float64(traced[1]).tobytes()
                    assert plain[2:] == traced[2:]
                    assert sum(r[2] for r in trace) == max(plain[3], 0) and (len(trace) == 0) == (plain[2] == lo.NOT_FITTED or fam.max_iter == 0)
                    assert all(r[1] == np.isnan(r[4]) and (not r[3] or r[2]) for r in trace)   # small implies accepted
                    n += 1
    assert n >= 200


# ------------------------------------------------------------------------------------------------------------------ what each family is for
@pytest.mark.parametrize("name", lc.HARD)
def test_hard_families_fail_pivots_and_climb(name):
    f = lc.fit(name)
    rec = _records(f)
    failed, rejected_on_cost = sum(r[1] for r in rec), sum(not r[1] and not r[2] for r in rec)
    climb = max(_rejections_then_acceptance(tr) for row in f.traces for tr in row)
    print(f"{name}: {len(rec)} passes, {sum(r[2] for r in rec)} accepted, {failed} pivot failures, {rejected_on_cost} rejected on cost; "
          f"longest climb {climb}; iterations at most {f.iters.max()}, passes at most {lc.passes(f).max()}")
    assert failed >= 50 and climb >= 3
    assert (f.status != lo.NOT_FITTED).all() and (f.status != lo.STALLED).all()


def test_some_family_rejects_on_cost():
    counts = {name: sum(not r[1] and not r[2] for r in _records(lc.fit(name))) for name in lc.HARD}
    print(counts)
    assert min(counts.values()) >= 5   # here every hard family does, not just one


@pytest.mark.parametrize("name", DEFAULT)
def test_lambda_returns_to_exactly_zero(name):
    """Every family fitted at the default max_iter; the limited ones end before lambda can come back, and tie_step's legs are easy."""
    f = lc.fit(name)
    assert any(_returns_to_zero(tr) for row in f.traces for tr in row)


def test_limited_has_both_statuses_at_the_boundary_counts():
    own = lc.fit("short").iters[:lc.LIMITED_FRAMES]
    assert (lc.fit("short").status[:lc.LIMITED_FRAMES] == lo.CONVERGED).all()
    assert tuple(lc.limited_counts()) == lc.LIMITED_COUNTS
    for m in sorted(set(lc.LIMITED_FIXED) | set(lc.LIMITED_COUNTS)):
        f = lc.fit(f"limited_{m}")
        done = own <= m
        # `small` is tested first: a leg that converges at its m-th acceptance is CONVERGED, one that needs m + 1 is not
        assert (f.status[done] == lo.CONVERGED).all() and np.array_equal(f.iters[done], own[done])
        assert (f.status[~done] == lo.OUT_OF_ITERATIONS).all() and (f.iters[~done] == m).all()
    for n in np.unique(own):
        assert (lc.fit(f"limited_{n}").status[own == n] == lo.CONVERGED).all()
        if n - 1 >= 1:
            assert (lc.fit(f"limited_{n - 1}").status[own == n] == lo.OUT_OF_ITERATIONS).all()
    at = lc.fit(f"limited_{int(np.median(own))}")
    assert (at.status == lo.CONVERGED).any() and (at.status == lo.OUT_OF_ITERATIONS).any()


@pytest.mark.parametrize("name", ["stalled", "stalled_free", "mixed", "mixed_free"])
def test_overflow_leg_stalls_after_seventeen_passes(name):
    """lambda = 0, then 1e-3 .. 1e12: sixteen damped values, the last of them LAMBDA_MAX itself (1e-3 x 10^15 is 1e12 exactly in
    float64, and the test is lam > LAMBDA_MAX), so seventeen passes, every one a failed first pivot."""
    fam, f = lc.families()[name], lc.fit(name)
    leg = lc.STALLED_LEG
    for t in range(len(fam.X)):
        if f.status[t, leg] == lo.NOT_FITTED:
            continue
        tr = f.traces[t][leg]
        assert f.status[t, leg] == lo.STALLED and f.iters[t, leg] == 0 and f.cost[t, leg] == np.inf
        assert len(tr) == 17 and all(r[1] and not r[2] for r in tr) and tr[0][0] == 0.0 and tr[-1][0] == lo.LAMBDA_MAX
        j = lo.leg_joints(leg)
        with np.errstate(all="ignore"):
            assert f.points[t, j].tobytes() == lo.replay(fam.X[t, j], fam.L[leg], None if fam.A is None else fam.A[leg]).tobytes()
    others = np.delete(f.status, leg, axis=1)
    assert (others != lo.STALLED).all() and (others == lo.CONVERGED).mean() >= 0.85


def test_no_seeded_leg_stalls_in_finite_arithmetic_but_a_constructed_one_does():
    for name in NAMES:
        fam, f = lc.families()[name], lc.fit(name)
        finite = (fam.L < 1e100).all(axis=1)
        if name != "edges":
            assert not (f.status[:, finite] == lo.STALLED).any(), name
    fam, f = lc.families()["edges"], lc.fit("edges")
    t, leg = lc.EDGE_LEGS["finite_stall"]
    tr = f.traces[t][leg]
    assert f.status[t, leg] == lo.STALLED and np.isfinite(f.cost[t, leg]) and np.isfinite(f.points[t, lo.leg_joints(leg)]).all()
    assert len(tr) == 17 and all(r[1] for r in tr)
    assert (np.delete(f.status, [t * 6 + leg]) != lo.STALLED).all()
    # ... and LAMBDA_MAX itself is tried: this leg's pivots fail through 1e11 and hold at 1e12, on a gradient of exactly zero
    t, leg = lc.EDGE_LEGS["lambda_max_tried"]
    tr = f.traces[t][leg]
    assert f.status[t, leg] == lo.CONVERGED and f.iters[t, leg] == 1 and len(tr) == 17
    assert all(r[1] for r in tr[:-1]) and tr[-1][0] == lo.LAMBDA_MAX and tr[-1][2] and tr[-1][3] and tr[-1][4] == 0.0


def test_mixed_waves_hold_every_kind_of_lane():
    for name in ("mixed", "mixed_free"):
        fam = lc.tiled(lc.families()[name], 75)
        f = lc.fit_family(fam)
        n = lc.passes(f).ravel()                      # lane g = 6 t + leg
        status = f.status.ravel()
        kinds = np.stack([status == lo.NOT_FITTED, (n >= 3) & (n <= 8) & (status == lo.CONVERGED), (n == 17) & (status == lo.STALLED), n > 20])
        assert (n[status == lo.NOT_FITTED] == 0).all()
        for g in range(0, len(n) - 63):               # every run of 64 lanes, a wave's among them
            assert kinds[:, g:g + 64].any(axis=1).all(), (name, g, kinds[:, g:g + 64].sum(axis=1))
        print(f"{name}: lanes per kind {kinds.sum(axis=1)} of {len(n)}, passes up to {n.max()}")


# ------------------------------------------------------------------------------------------------------------------ ties and thresholds
def test_tie_poses_tie():
    fam = lc.families()["edges"]
    seen, negative_zeros = set(), 0
    for t in range(4):
        for leg in range(6):
            p0, tt, d = lo.start(fam.X[t, lo.leg_joints(leg)])
            s = np.concatenate([tt[:1], tt[1:] - tt[:-1]])
            for k in range(4):
                a = np.abs(d[k])
                tied = tuple(int(c) for c in np.nonzero(a == a.min())[0])
                if t < 3 or k == 0:
                    assert len(tied) >= 2, (t, leg, k, d[k])
                if len(tied) >= 2:
                    assert int(np.argmin(a)) == tied[0]          # the model: the lowest index among the tied
                    seen.add((tied, tuple(int(c) for c in np.sign(d[k]))))
                    negative_zeros += int((np.signbit(s[k]) & (s[k] == 0.0)).sum())
    two = {k for k in seen if len(k[0]) == 2}
    three = {k for k in seen if len(k[0]) == 3}
    print(f"{len(two)} axis directions, {len(three)} diagonals, {negative_zeros} components of -0.0")
    assert len(two) == 6 and len(three) == 8 and negative_zeros == 12
    assert {k[0] for k in two} == {(1, 2), (0, 2), (0, 1)}


def test_named_edge_legs_take_their_branch():
    fam, f = lc.families()["edges"], lc.fit("edges")
    got = {name: (int(f.status[t, leg]), int(f.iters[t, leg])) for name, (t, leg) in lc.EDGE_LEGS.items()}
    print(got)
    P = {name: fam.X[t, lo.leg_joints(leg)] for name, (t, leg) in lc.EDGE_LEGS.items()}
    # the thresholds, a factor of two either side of TINY
    for name, ratio, fitted in (("below_tiny", 0.5e-18, False), ("above_tiny", 2e-18, True)):
        tt = P[name][1:] - P[name][0]
        s3 = tt[2] - tt[1]
        r = (s3 @ s3) / max(x @ x for x in tt)
        assert abs(r / ratio - 1.0) < 1e-6 and (got[name][0] != lo.NOT_FITTED) == fitted, (name, r)
    assert got["above_tiny"][0] == lo.CONVERGED
    # straight legs: the reachable one comes back with no cost, the one twice too long ends straight along its own line
    assert got["straight"] == (lo.CONVERGED, 1) and f.cost[lc.EDGE_LEGS["straight"]] <= lc.RIGID_COST
    t, leg = lc.EDGE_LEGS["too_long"]
    out = f.points[t, lo.leg_joints(leg)]
    u = (P["too_long"][4] - P["too_long"][0]) / np.linalg.norm(P["too_long"][4] - P["too_long"][0])
    assert got["too_long"][0] == lo.CONVERGED and np.abs(np.diff(out, axis=0) - fam.L[leg][:, None] * u).max() <= 1e-12
    # antiparallel segments: exactly so in the start directions, and the first pivots fail on the folded chain's curvature
    t, leg = lc.EDGE_LEGS["antiparallel"]
    d = lo.start(P["antiparallel"])[2]
    assert all(abs(d[k] @ d[k + 1] + 1.0) <= 4e-16 for k in range(3)) and f.traces[t][leg][0][1] and got["antiparallel"][0] == lo.CONVERGED
    assert np.array_equal(P["tip_on_anchor"][4], P["tip_on_anchor"][0]) and got["tip_on_anchor"][0] == lo.CONVERGED


def test_tie_step_leg_separates_the_lowest_index_from_the_highest(monkeypatch):
    fam, f = lc.families()["tie_step"], lc.fit("tie_step")
    t, leg = lc.TIE_SENSITIVE
    P = fam.X[t, lo.leg_joints(leg)]
    d = lo.start(P)[2]
    assert d[0][0] == d[0][1] == d[0][2] > 0.0
    low = f.traces[t][leg]
    assert (f.status[t, leg], f.iters[t, leg]) == (lo.CONVERGED, 1) and len(low) == 1 and 0.84e-9 < low[0][4] < 0.86e-9
    monkeypatch.setattr(lo, "tangent_basis", _highest_index_basis)
    high = []
    out = lo.fit_leg(P, fam.L[leg], trace=high)
    print(f"largest tangent coordinate of the first step: {low[0][4]:.4e} with the lowest index, {high[0][4]:.4e} with the highest")
    assert out[2:] == (lo.CONVERGED, 2) and len(high) == 2 and high[0][4] > 1.12e-9 and high[0][2] and not high[0][3]


# ------------------------------------------------------------------------------------------------------------------ the oracle against itself
@pytest.mark.parametrize("name", NAMES)
def test_oracle_paths_agree_as_measured(name):
    differ, dp, dc = lc.compare_paths(name)
    fitted = int((lc.fit(name).status != lo.NOT_FITTED).sum())
    n = int(differ.sum())
    print(f'    "{name}": ({n}, {dp:.3e}, {dc:.3e}),   # of {fitted} fitted legs')
    if name == "tie_step":   # max |delta| is a norm of tangent COORDINATES: within 15 % of TOL the basis is part of the model, by design
        assert np.array_equal(np.argwhere(differ), [list(lc.TIE_SENSITIVE)])
    else:
        assert n <= lc.ORACLE_FLIP_CAP * fitted
    want = lc.MEASURED[name]
    assert n == want[0]
    for got, pinned in ((dp, want[1]), (dc, want[2])):   # a few units in the last place: a drift beyond a factor of two either way fails
        assert pinned / 2.0 <= got <= max(pinned * 2.0, 4.5e-16), (got, pinned)   # 4.4e-16: one unit in the last place at scale 1
    assert lc.ORACLE_FLIP_CAP * 2 <= lc.FLIP_CAP
