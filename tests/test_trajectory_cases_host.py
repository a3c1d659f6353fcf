"""CPU certificate of the families tests/test_gpu_trajectory_sweep.py runs on the device (tests/trajectory_cases.py, DESIGN.md section 24,
"swept"): each family does what its name says, every chain a GPU test asserts exactly is firm -- tests/trajectory_oracle.fit takes the same
accept / cost-reject / pivot-reject decision on every trial in float64, in numpy.longdouble and in float64 with numpy.linalg.solve on
the dense matrix in place of the banded substitution -- and the path-to-path differences and decision margins are pinned, so that a later
change to a family cannot quietly make it chaotic.  The oracle alone; nothing here touches a device."""
import numpy as np
import pytest

import trajectory_cases as tc
import trajectory_oracle as to
from deepfly3d_amd import config

SLACK, TOL, MAX_ITER = config.TRAJECTORY_SLACK, config.TRAJECTORY_STEP_TOL, config.TRAJECTORY_MAX_ITER
# the largest |X - X'| (mm) between two of the three paths over a family's firm chains may not pass SPREAD: about four times what the
# oracle gives today (4.9e-11 rejected, 9.8e-13 rejected_clean, 7.7e-14 out_of_iterations, 1.4e-13 mixed, at most 1.8e-15 elsewhere)
SPREAD = {"rejected": 2e-10, "rejected_clean": 4e-12, "out_of_iterations": 4e-13, "mixed": 6e-13}
SPREAD_ELSEWHERE = 1e-14
# no cost decision of a firm chain is nearer to its threshold than 0.99 SLACK (relative to the cost): the nearest are trials whose cost
# equals the cost before to the last bit, which SLACK exists to accept -- rounding moves a cost by 1e-16 of itself, four orders less;
# no step decision is nearer to STEP_TOL than 1 % of it (the nearest today: 1.7 % in cameras2, 2.8 % in cost_stalled's chain 0)
COST_MARGIN, STEP_MARGIN = 0.99 * SLACK, 0.01
# (trials, rejected on cost, rejected at a pivot) of float64, per chain of the small families
TRIALS = {"rejected": [(35, 0, 0), (119, 66, 0)], "rejected_clean": [(11, 0, 0), (16, 6, 0)], "out_of_iterations": [(300, 0, 0), (90, 0, 0)],
          "pivot_stall": [(16, 0, 16), (16, 0, 16)], "nan_cost_stall": [(16, 16, 0), (3, 0, 0)], "per_joint_lambda": [(11, 0, 0), (26, 0, 0)],
          "mixed": [(82, 45, 0), (300, 0, 0), (90, 0, 0), (16, 0, 16), (0, 0, 0)]}
ENDS = {"rejected": [to.CONVERGED] * 2, "rejected_clean": [to.CONVERGED] * 2, "out_of_iterations": [to.OUT_OF_ITERATIONS, to.CONVERGED],
        "pivot_stall": [to.STALLED] * 2, "nan_cost_stall": [to.STALLED, to.CONVERGED], "per_joint_lambda": [to.CONVERGED] * 2,
        "cost_stalled": [to.CONVERGED, to.STALLED],
        "mixed": [to.CONVERGED, to.OUT_OF_ITERATIONS, to.CONVERGED, to.STALLED, to.CONVERGED]}


def _counts(fam):
    """[(trials, cost rejections, pivot rejections)] of the float64 oracle on the whole launch."""
    d = tc.decisions(fam.P, fam.px, fam.X0, fam.lam, fam.huber, fam.max_gap, paths=("float64",))
    return [(len(s), s.count("c"), s.count("p")) for s in d.strings["float64"]], d


@pytest.mark.parametrize("name", tc.SWEEP_FAMILIES)
def test_firm_chains_are_firm_and_pinned(name):
    fam, cert = tc.sweep(name), tc.certificate(name)
    J = fam.px.shape[2]
    assert sorted(fam.firm + fam.structural) == sorted(set(fam.firm + fam.structural)) and all(0 <= j < J for j in fam.firm + fam.structural)
    assert fam.px.shape[1] <= 40 and J <= 5 or name == "long" or name.startswith("segments")
    assert np.array_equal(cert.whole["fit_status"] != to.CONVERGED, (cert.whole["status"] == 4).any(axis=0))
    if not fam.firm:
        assert cert.three is None
        return
    d = cert.three
    print(f"{name}: firm chains {len(fam.firm)} of {J}, largest |X - X'| between paths {d.spread.max():.2e} mm, smallest cost margin "
          f"{d.cost_margin.min():.2e}, smallest step margin {d.step_margin.min():.2e}, trials {min(map(len, d.strings['float64']))} .. "
          f"{max(map(len, d.strings['float64']))}")
    assert d.firm.all(), (name, np.nonzero(~d.firm)[0])
    assert all(np.array_equal(d.fit_status[p], d.fit_status["float64"]) for p in tc.PATHS)
    # a chain's fit is its own: alone with the other firm chains it takes the decisions it takes in the whole launch
    whole = tc.result_of(cert.whole, fam.firm)
    for key in ("X", "status", "iterations", "cost", "counts", "fit_status"):
        assert np.array_equal(whole[key], d.results["float64"][key], equal_nan=True), (name, key)
    assert d.spread.max() <= SPREAD.get(name, SPREAD_ELSEWHERE)
    assert d.cost_margin.min() >= COST_MARGIN and d.step_margin.min() >= STEP_MARGIN
    assert tc.point_bar(name) == max(16.0 * d.spread.max(), TOL)


@pytest.mark.parametrize("name", sorted(TRIALS))
def test_small_families_do_what_their_names_say(name):
    fam = tc.sweep(name)
    counts, d = _counts(fam)
    r = d.results["float64"]
    print(name, counts, r["fit_status"].tolist(), r["iterations"].tolist())
    assert counts == TRIALS[name] and r["fit_status"].tolist() == ENDS[name]
    assert [c[0] - c[1] - c[2] for c in counts] == r["iterations"].tolist()
    for j, end in enumerate(ENDS[name]):
        active = r["active"][:, j]
        assert ((r["status"][:, j] == 4) == (active & (end != to.CONVERGED))).all()
        assert r["counts"][j, 4] == (active.sum() if end != to.CONVERGED else 0)
    assert fam.px.shape[1] <= 40


def test_out_of_iterations_is_no_near_miss():
    fam = tc.sweep("out_of_iterations")
    r = to.fit(fam.P, fam.px, fam.X0, fam.lam, fam.huber, fam.max_gap, max_iter=5000)
    trace = []
    to.fit(fam.P, fam.px[:, :, :1], fam.X0[:, :1], fam.lam[:1], fam.huber, fam.max_gap, max_iter=5000, trace=trace)
    print(f"unlimited: {len(trace)} trials, {r['iterations'][0]} accepted")
    assert r["fit_status"][0] == to.CONVERGED and len(trace) >= 2 * MAX_ITER
    # the mixed launch's chain 1 is the same chain
    mixed = tc.sweep("mixed")
    assert np.array_equal(mixed.px[:, :, 1], fam.px[:, :, 0]) and np.array_equal(mixed.X0[:, 1], fam.X0[:, 0]) and mixed.lam[1] == fam.lam[0]
    assert mixed.huber == fam.huber and mixed.max_gap == fam.max_gap


def test_the_structural_stalls():
    """Their certificate is the float64 oracle and an argument, not the three paths: numpy.longdouble does not overflow at 3.4e308 (so
    neither lambda k1 nor B - A is infinite there) and its 10 mu passes MU_MAX one trial earlier.  pivot_stall: lambda k1 = -inf beside
    every pair of centres; whichever of the two rows is eliminated first, its multiplier -inf / p is infinite (or NaN), the other row's
    pivot becomes inf - inf = NaN, and NaN > 0 is false in any order of elimination -- every trial is rejected at a pivot, whatever mu.
    nan_cost_stall: the start of the bridged frame is A + (B - A) w with B - A = -inf, so the triples around it hold inf - inf, the cost
    of the start is NaN, every trial's cost is NaN and NaN <= x is false -- every trial is rejected on cost, and E stays the start's NaN.
    Sixteen rejections take mu from 1e-3 past MU_MAX = 1e12."""
    assert config.TRAJECTORY_MU_INIT * 10.0 ** 16 > config.TRAJECTORY_MU_MAX >= config.TRAJECTORY_MU_INIT * 10.0 ** 15
    for name, chains, letter in (("pivot_stall", (0, 1), "p"), ("nan_cost_stall", (0,), "c"), ("mixed", (3,), "p")):
        fam = tc.sweep(name)
        assert fam.structural == chains and np.isfinite(fam.lam).all() and (fam.lam >= 0.0).all()
        counts, d = _counts(fam)
        r = d.results["float64"]
        active, anchor = r["active"], r["anchor"]
        start = to.start_points(fam.X0, anchor, active)
        for j in chains:
            assert d.strings["float64"][j] == letter * 16 and r["fit_status"][j] == to.STALLED and r["iterations"][j] == 0
            assert active[:, j].any() and np.array_equal(r["X"][:, j].view(np.int64), start[:, j].view(np.int64))
            assert np.array_equal(r["cost"][j, :1].view(np.int64), r["cost"][j, 1:].view(np.int64))
        if name == "nan_cost_stall":
            assert np.isnan(r["cost"][0]).all() and np.isinf(start[10, 0]).all() and np.isfinite(np.delete(start[:, 0], 10, axis=0)).all()
            assert np.isfinite(r["cost"][1]).all()
        else:
            with np.errstate(over="ignore"):
                assert np.isinf(fam.lam[list(chains)] * -2.0).all() and np.isfinite(r["cost"][list(chains), 0]).all()


def test_cost_stalled_is_not_firm_on_purpose():
    fam = tc.sweep("cost_stalled")
    d = tc.decisions(fam.P, fam.px, fam.X0, fam.lam, fam.huber, fam.max_gap)
    s = d.strings["float64"][1]
    print(f"cost_stalled chain 1: trials {[len(d.strings[p][1]) for p in tc.PATHS]}, ends {[int(d.fit_status[p][1]) for p in tc.PATHS]}, "
          f"paths apart by {d.spread[1]:.2e} mm")
    assert fam.firm == (0,) and d.firm[0] and not d.firm[1]
    assert d.fit_status["float64"].tolist() == ENDS["cost_stalled"] and s.count("c") > 50 and s.count("p") == 0 and s.endswith("c")
    assert d.spread[1] > TOL                            # the paths end further apart than the iteration's own tolerance


def test_mixed_ends_in_every_way_with_a_lambda_per_chain():
    fam = tc.sweep("mixed")
    r = tc.certificate("mixed").whole
    assert len(set(fam.lam.tolist())) == 4 and fam.lam[0] != fam.lam[1]
    assert not r["active"][:, 4].any() and r["counts"][4].tolist() == [24, 0, 0, 0, 0]
    assert set(r["fit_status"].tolist()) == {to.CONVERGED, to.OUT_OF_ITERATIONS, to.STALLED}


def test_long_and_segments_hold_what_the_sweep_needs():
    fam, r = tc.sweep("long"), tc.certificate("long").whole
    T = fam.px.shape[1]
    assert T == 1025 and -(-T // 3) == 342 > 256 and -(-T // 256) == 5 and config.trajectory_block_frames(T) == 33
    status = r["status"][:, 0]
    assert (status[:7] == 0).all() and (status[1016:] == 0).all() and (status[700:706] == 3).all() and set(np.unique(status)) == {0, 1, 2, 3}
    runs = np.flatnonzero(np.diff(np.concatenate([[0], (status == 2).astype(int), [0]]))).reshape(-1, 2)
    assert len(runs) == 4 and all(b - a == tc.GAP_LEN and a // 5 != (b - 1) // 5 for a, b in runs)      # each crosses setup chunks
    assert (r["fit_status"] == to.CONVERGED).all()
    firsts, lasts, lengths, gaps = set(), set(), set(), set()
    for max_gap in (0, 1, 2, 5):
        fam, r = tc.sweep(f"segments{max_gap}"), tc.certificate(f"segments{max_gap}").whole
        assert fam.px.shape[1:3] == (64, 64) and fam.max_gap == max_gap and (r["fit_status"] == to.CONVERGED).all()
        active = np.zeros((64, 64), bool)
        for j in range(64):
            a = r["anchor"][:, j]
            firsts.add(bool(a[0])), lasts.add(bool(a[-1]))
            at = np.flatnonzero(a)
            gaps |= set((np.diff(at) - 1).tolist())
            edges = np.flatnonzero(np.diff(np.concatenate([[0], a.astype(int), [0]]))).reshape(-1, 2)
            lengths |= set((edges[:, 1] - edges[:, 0]).tolist())
            for first, last in to.segments_loop(a, max_gap):
                active[first : last + 1, j] = True
        assert np.array_equal(active, r["active"])
        assert {max_gap, max_gap + 1} <= gaps and (r["counts"][:, 0] > 0).any()
    assert firsts == {True, False} and lasts == {True, False} and {2, 3} <= lengths
    for ncam in (2, 8):
        fam = tc.sweep(f"cameras{ncam}")
        assert fam.P.shape == (ncam, 3, 4) and to.views(fam.px).sum(axis=0).min() == min(ncam, 3)


def test_the_hooks_change_nothing_when_absent():
    fam = tc.sweep("rejected_clean")
    plain = to.fit(fam.P, fam.px, fam.X0, fam.lam, fam.huber, fam.max_gap)
    traced = to.fit(fam.P, fam.px, fam.X0, fam.lam, fam.huber, fam.max_gap, solve=to.banded_solve, trace=[])
    assert plain.keys() == traced.keys() and all(np.array_equal(plain[k], traced[k], equal_nan=True) for k in plain)
