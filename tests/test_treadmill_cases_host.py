"""CPU certificate of the families tests/test_gpu_treadmill_sweep.py runs on the device (tests/treadmill_cases.py, DESIGN.md section 21,
"swept"): every family does what its name says (status, count, the first step lengths), every Cholesky pivot the oracle compares with
its floor is firm -- accepted at 100 times the floor or more, refused at a hundredth of it or less, with exact sums and with the
kernel's order of summation --, so that no status the GPU test asserts hangs on rounding, and the blind spot the sweep closes is
pinned by mutants of the Gauss-Newton step.  The oracle alone; nothing here touches a device."""
import numpy as np
import pytest

import gait_oracle as go
import pose_repair_oracle as pr
import treadmill_cases as tc
import treadmill_oracle as to

FIRM = 100.0
TOTALS = (to.exact_sum, to.slice_sum)
# (count, status with a free radius, status with the known radius) of every fit case
EXPECT = {"n1": (1, 1, 1), "n2": (2, 1, 1), "n3": (3, 1, 2), "n4": (4, 0, 0), "n5": (5, 0, 0), "spread3": (3, 1, 2), "spread4": (4, 0, 0),
          "spread5": (5, 0, 0), "colinear3": (3, 1, 3), "zero_mean3": (3, 1, 1), "coplanar4": (4, 1, 2), "identical8": (8, 1, 3),
          "plane40_1e-7": (40, 1, 2), "plane40_1e-3": (40, 0, 0), "radius2": (48, 0, 0), "radius6": (48, 0, 0), "flat_circle": (2077, 1, 2)}
# the first four Gauss-Newton step lengths of the far starts (mm): long, then a contraction that the bars may rely on
FIRST_STEPS = {"radius2": (1.18221, 0.0684038, 0.0106452, 0.00188987), "radius6": (3.54662, 0.236977, 0.00475157, 0.000567866),
               "flat_circle": (1.06756, 0.169236, 0.00540571, 5.44097e-06)}
ALL_FITS = sum(tc.FAMILIES.values(), ())


def _firm(seen, name):
    """The (pivot, floor) pairs are firm; returns (the smallest accepted pivot over its floor, the largest refused one over its floor)."""
    accepted = [p / f for p, f in seen if p > f]
    refused = [(p / f if f > 0.0 else 0.0) for p, f in seen if not p > f]
    assert all(f >= 0.0 and np.isfinite(p) for p, f in seen), name
    assert all(a >= FIRM for a in accepted) and all(r <= 1.0 / FIRM for r in refused), (name, seen)
    return min(accepted, default=np.inf), max(refused, default=-np.inf)


@pytest.mark.parametrize("name", ALL_FITS)
def test_fit_cases_do_what_their_names_say_and_every_pivot_is_firm(name):
    case = tc.fit_case(name)
    count, free, known = EXPECT[name]
    for total in TOTALS:
        for radius, status in ((None, free), (case.radius, known)):
            seen, fit = tc.pivot_decisions(case, radius, total)
            assert fit["count"] == count and fit["status"] == status, (name, radius, total.__name__)
            low, high = _firm(seen, name)
            # 64 steps take no decision that 8 did not take differently: the pivots stay firm to the end
            _firm(tc.pivot_decisions(case, radius, total, 64)[0], name)
            if total is to.exact_sum:
                print(f"{name}, radius {radius}: status {status}, {len(seen)} pivots, accepted >= {low:.3g} floors, refused <= {high:.3g} floors")
    assert case.b.flags.writeable is False and case.states.dtype == np.int32


def test_counts_and_degenerate_by_hand():
    for n in range(1, 6):
        case = tc.fit_case(f"n{n}")
        assert case.b.shape == (1, 6, 3) and to.samples(case.b, case.states)[0].tolist() == [k < n for k in range(6)]
        on = to.samples(case.b, case.states)
        assert np.allclose(np.linalg.norm(case.b[on] - tc.CENTER, axis=-1), tc.RADIUS, rtol=0, atol=1e-14)
    for n in (3, 4, 5):
        case = tc.fit_case(f"spread{n}")
        on = to.samples(case.b, case.states)
        assert case.b.shape == (5, 6, 3) and on.sum(axis=1).tolist() == [1] * n + [0] * (5 - n)
        # the other lanes: swing, unknown, and stance tips that are no numbers
        assert {-1, 0, 1} <= set(case.states[~on].tolist()) and (~np.isfinite(case.b[(case.states == 0) & ~on])).any(axis=-1).all()
    # four samples on a sphere: the sphere itself
    fit = to.fit_ball(*tc.fit_case("n4")[:2])
    assert np.linalg.norm(fit["center"] - tc.CENTER) <= 1e-12 and abs(fit["radius"] - tc.RADIUS) <= 1e-12 and fit["rms"] <= 1e-12
    # three samples and a known radius: from beyond their mean onto one of the two spheres through them
    for name in ("n3", "spread3"):
        case = tc.fit_case(name)
        fit = to.fit_ball(*case)
        pts = case.b[to.samples(case.b, case.states)]
        assert np.abs(np.linalg.norm(pts - fit["center"], axis=1) - case.radius).max() <= 1e-12 and fit["steps"][0] > 0.5 > 1e-9 > fit["steps"][-1]
    # the refusals: by the count, by the mean, by a pivot of the 4 x 4 fit, by a pivot of the first step
    case = tc.fit_case("zero_mean3")
    for total in TOTALS:
        s = to.ball_sums(case.b, case.states, total)
        assert s[0] == 3.0 and not s[1:4].any() and to.start_below(s, case.radius) is None
    pts = tc.fit_case("colinear3").b[to.samples(*tc.fit_case("colinear3")[:2])]
    assert np.linalg.matrix_rank(pts - pts.mean(axis=0), tol=1e-12) == 1 and np.linalg.matrix_rank(pts, tol=1e-12) == 2   # a line off the origin
    pts = tc.fit_case("coplanar4").b[to.samples(*tc.fit_case("coplanar4")[:2])]
    assert np.linalg.matrix_rank(pts - pts.mean(axis=0), tol=1e-12) == 2 and np.ptp(pts[:, 2]) > 0.1   # a tilted plane
    pts = tc.fit_case("identical8").b[to.samples(*tc.fit_case("identical8")[:2])]
    assert len(pts) == 8 and not np.ptp(pts, axis=0).any()
    for name, status in (("colinear3", 3), ("identical8", 3)):
        seen, fit = tc.pivot_decisions(tc.fit_case(name), tc.RADIUS)
        assert fit["status"] == status == (to.REFUSED | to.START_BELOW) and fit["steps"] == []   # the first step is the refused one
    # the two planes: the same 4 x 4 pivot either side of its floor
    low = tc.pivot_decisions(tc.fit_case("plane40_1e-7"), None)[0][-1]
    high = tc.pivot_decisions(tc.fit_case("plane40_1e-3"), None)[0][-1]
    print(f"plane40: the last pivot is {low[0] / low[1]:.3g} floors at 1e-7 and {high[0] / high[1]:.3g} floors at 1e-3")
    assert low[0] > 0.0 and low[0] / low[1] <= 1e-3 and high[0] / high[1] >= 1e3


@pytest.mark.parametrize("name", tc.FAR_START)
def test_far_starts_take_long_first_steps_and_then_contract(name):
    case = tc.fit_case(name)
    for total in TOTALS:
        fit = to.fit_ball(*case, total=total)
        assert fit["steps"][:4] == pytest.approx(FIRST_STEPS[name], rel=1e-4)
    fit = to.fit_ball(*case, iterations=64)
    assert fit["steps"][0] > 1.0 and fit["steps"][-1] <= 1e-15 and np.isfinite(to.known_radius_bar(case.b, case.states, fit))   # (asserts the rate)
    if name == "flat_circle":
        n = 6 * len(case.b)
        assert -(-n // to.SLICE) == 3 and all(to.samples(case.b, case.states).reshape(-1)[k * to.SLICE:(k + 1) * to.SLICE].sum() > 20 for k in range(3))
        assert fit["status"] == to.START_BELOW and np.linalg.norm(fit["center"] - tc.CENTER) <= 1e-9
    else:
        assert 40 <= fit["count"] <= 60 and np.array_equal(case.b, tc.fit_case("radius6" if name == "radius2" else "radius2").b, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ the blind spot
def _zero_yz(g):
    g = g.copy()
    g[4] = 0.0
    return g


def _swap_xy_xz(g):
    g = g.copy()
    g[1], g[2] = g[2], g[1]
    return g


def _doubled(g):
    g = g.copy()
    g[:6] *= 2.0
    return g


def _yz_nine_tenths(g):
    g = g.copy()
    g[4] *= 0.9
    return g


MUTANTS = (_zero_yz, _swap_xy_xz, _doubled)


def _start(case):
    s = to.ball_sums(case.b, case.states)
    fit = to._algebraic(s)
    return fit[0] if fit is not None else to.start_below(s, case.radius)


@pytest.mark.parametrize("name", tc.FAR_START)
def test_one_step_sees_every_mutant(name):
    """A step matrix with `uy uz` zeroed, with `ux uy` and `ux uz` swapped, or doubled: each misses step_bar on every step of every far
    start that is longer than 1e-9 (below that a step is rounding, known_radius_bar's convention, and a wrong matrix times a right side
    of rounding is rounding) -- the first four steps of every input at the least, by a factor of 1e6 or more.  The kernel's order of
    summation, which is what the bar is for, stays below a hundredth of it."""
    case = tc.fit_case(name)
    b, states, R = case
    c, checked = _start(case), 0
    for k in range(1, 8):
        want, _ = to.gauss_newton_step(b, states, c, R)
        bar = to.step_bar(b, states, c, R)
        length = float(np.linalg.norm(want - c))
        kernel = float(np.linalg.norm(to.gauss_newton_step(b, states, c, R, to.slice_sum)[0] - want))
        assert kernel <= 0.01 * bar
        off = []
        for mutant in MUTANTS:
            got, _ = to.gauss_newton_step(b, states, c, R, alter=mutant)
            off.append(np.inf if got is None else float(np.linalg.norm(got - want)))   # a refused step is NaN on the device
        print(f"{name} step {k}: length {length:.3g}, bar {bar:.3g}, the kernel's order {kernel / bar:.2g} of it, the mutants {[f'{o / bar:.3g}' for o in off]}")
        if length > 1e-9:
            assert min(off) > 1e6 * bar if k <= 4 else min(off) > bar
            checked += 1
        c = want
    assert checked >= 4


def test_a_converged_comparison_cannot_see_the_matrix():
    """On the tips and states of tests/test_gpu_treadmill.py at T = 257, the known-radius comparison there.  The fixed point of
    c <- c + N^-1 g is g = 0 whatever N: after 64 steps the first two mutants end inside known_radius_bar of the true oracle (2.2e-16
    and 4.4e-16 against 8.9e-14), and all that a wrong N changes is the rate.  After the default 8 steps the two are still on their
    way (2.7e-8 and 2.4e-10 from the true centre, at their rates of about 0.3 and 0.15 a step against the true 1e-3: these two the
    8-step comparison does see at this size, by their slowness alone; at T = 2 049 it sees the zeroed sum (4.6e-10 against 2.8e-13)
    and not the swap (4.9e-17)), and a sum that is wrong by a tenth ends 8 steps inside the bar at both sizes.  The same mutants are
    1e9 bars and more off after one step of a far start (test_one_step_sees_every_mutant)."""
    import test_gpu_treadmill as tg

    for T, seen_at_8 in ((257, (True, True)), (2049, (True, False))):
        X, F, states = tg._inputs(T)
        b, _ = to.body_tips(X, tg.FPS, F, to.coxa_medians(X), tg.W)
        for iterations, mutants in ((64, (_zero_yz, _swap_xy_xz)), (8, (_yz_nine_tenths,))):
            true = to.fit_ball(b, states, tg.RADIUS, iterations)
            bar = to.known_radius_bar(b, states, true)
            for mutant in mutants:
                fit = to.fit_ball(b, states, tg.RADIUS, iterations, alter=mutant)
                off = float(np.linalg.norm(fit["center"] - true["center"]))
                print(f"T = {T}, {iterations} steps, {mutant.__name__}: {off:.2e} from the true oracle, {off / bar:.2g} of known_radius_bar")
                assert fit["status"] == 0 and off <= bar
        true = to.fit_ball(b, states, tg.RADIUS)
        bar = to.known_radius_bar(b, states, true)
        for mutant, seen in zip((_zero_yz, _swap_xy_xz), seen_at_8):
            off = float(np.linalg.norm(to.fit_ball(b, states, tg.RADIUS, alter=mutant)["center"] - true["center"]))
            print(f"T = {T}, 8 steps, {mutant.__name__}: {off:.2e} from the true oracle, {off / bar:.2g} of known_radius_bar")
            assert (off > bar) == seen


def test_the_hooks_change_nothing_when_absent():
    case = tc.fit_case("radius6")
    plain = to.fit_ball(*case)
    hooked = to.fit_ball(*case, alter=lambda g: g, seen=[])
    assert all(np.array_equal(np.asarray(plain[k], dtype=np.float64), np.asarray(hooked[k], dtype=np.float64), equal_nan=True) for k in plain)
    c = _start(case)
    for k in range(3):   # gauss_newton_step is fit_ball's loop body
        c, g = to.gauss_newton_step(case.b, case.states, c, case.radius)
    assert np.array_equal(c, to.fit_ball(*case, iterations=3)["center"]) and np.array_equal(g, to.fit_ball(*case, iterations=3)["last"])


# ------------------------------------------------------------------------------------------------------------------ rotation, path, carry
def test_rotation_frames_and_their_pivots():
    b, v, states, usable = tc.rotation_case()
    r = {m: to.ball_rotation(b, v, states, tc.CENTER, tc.RADIUS, m) for m in range(2, 7)}
    assert np.array_equal(r[2]["legs"], usable)
    for m in range(2, 7):
        assert {m - 1, m, 6} <= set(usable[:12].tolist())
        solved = np.isfinite(r[m]["rotation"]).all(axis=1)
        expect = usable >= m
        expect[tc.ROTATION_FRAMES["parallel"]] = False
        assert np.array_equal(solved, expect), m
    t = tc.ROTATION_FRAMES["velocity_nan"]
    assert (states[t, :3] == 0).all() and np.isfinite(b[t, :3]).all() and np.isnan(v[t, 1]).sum() == 1 and usable[t] == 2
    # every pivot of every frame the device solves (two usable legs or more) is firm
    use, M, _, _, _ = to.rotation_system(b, v, states, tc.CENTER)
    pivots = to.solve3_pivots(M)
    floor = to.FRAME_PIVOT_MIN * (M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2])
    for t in np.nonzero(usable >= 2)[0]:
        ratio = pivots[t] / floor[t]
        if t == tc.ROTATION_FRAMES["parallel"]:
            assert ratio[0] >= FIRM and ratio[1] >= FIRM and ratio[2] <= 1.0 / FIRM, ratio
        else:
            assert (ratio >= FIRM).all(), (t, ratio)
    solved = (usable >= 2) & (np.arange(len(usable)) != tc.ROTATION_FRAMES["parallel"])
    print(f"rotation: accepted pivots >= {(pivots / floor[:, None])[solved].min():.3g} floors, the parallel frame's last "
          f"{pivots[tc.ROTATION_FRAMES['parallel'], 2] / floor[tc.ROTATION_FRAMES['parallel']]:.3g}")
    # the balls: a centre at the body's origin has no direction to the fly; a radius that is no number refuses everything but `legs`
    at_origin = to.ball_rotation(b, v, states, np.zeros(3), tc.RADIUS)
    M = to.rotation_system(b, v, states, np.zeros(3))[1]      # (seen from the origin no three radii are parallel: every frame is solved)
    assert (to.solve3_pivots(M)[usable >= 2] >= FIRM * to.FRAME_PIVOT_MIN * (M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2])[usable >= 2, None]).all()
    assert np.isfinite(at_origin["rotation"]).all(axis=1).sum() >= 15 and np.isnan(at_origin["fictive"]).all()
    assert to.fictive_path(at_origin["fictive"], tc.FPS)["skipped"] == len(b)
    for name in ("nan_radius", "inf_radius"):
        ball = tc.ROTATION_BALLS[name]
        bad = to.ball_rotation(b, v, states, np.array(ball[:3]), ball[3])
        assert np.isnan(bad["rotation"]).all() and np.isnan(bad["fictive"]).all() and np.isnan(bad["residual"]).all() and np.array_equal(bad["legs"], usable)


def test_path_cases():
    f = tc.path_case("edges")
    bad = ~np.isfinite(f).all(axis=1)
    runs = np.flatnonzero(np.diff(np.concatenate([[0], bad.astype(int), [0]]))).reshape(-1, 2)
    assert [tuple(r) for r in runs.tolist()] == [(0, 3), (250, 256), (300, 303), (512, 520), (760, 775), (1024, 1280)]
    assert 256 % to.SCAN_BLOCK == 0 and 512 % to.SCAN_BLOCK == 0 and 760 // to.SCAN_BLOCK != 774 // to.SCAN_BLOCK and (1024, 1280) == (4 * 256, 5 * 256)
    assert [int((~np.isfinite(f[300 + c])).sum()) for c in range(3)] == [1, 1, 1] and np.isinf(f[300:303]).sum() == 3
    p = to.fictive_path(f, tc.FPS)
    assert p["skipped"] == bad.sum() and not p["path"][:4].any() and p["path"][4].any()
    p = to.fictive_path(tc.path_case("large_yaw"), tc.FPS)
    assert len(p["path"]) == 512 and p["path"][-1, 2] == pytest.approx(511 * 200.0) and p["path"][-1, 2] > 1e5
    for T in (65535, 65536, 131073):
        f = tc.path_case(f"T{T}")
        assert f.shape == (T, 3) and 0 < (~np.isfinite(f).all(axis=1)).sum() == -(-T // 97)
    f = tc.path_case("carry3")
    moving = f.any(axis=1)
    assert len(f) == tc.T3 == 2 * 256 * 256 + 1 and moving[:tc.CHUNK].all() and not moving[tc.CHUNK:-1].any() and moving[-1]


def test_three_chunk_inputs():
    assert tc.T3 == 131073 and -(-tc.T3 // to.SCAN_BLOCK) == 2 * 256 + 1 and -(-tc.T3_FILL // to.SCAN_BLOCK) == 2 * 256 + 2
    vel = tc.gait_carry_velocity(go.ON, go.OFF)
    u = vel[..., 0]
    decisive = np.isnan(u) | (u > go.ON) | (u < go.OFF)
    assert decisive.sum(axis=0).tolist() == [1] * 6 and not decisive[tc.CHUNK:].any()
    assert sorted(np.nonzero(decisive)[0].tolist()) == sorted(t for _, t, _ in tc.GAIT_DECISIVE)
    states = go.states_of(u[:tc.CHUNK + 1], go.ON, go.OFF)      # (the whole recurrence runs beside the device, in the GPU test)
    assert states[-1].tolist() == [1, 0, 1, -1, 0, 1]
    for T in (tc.T3, tc.T3_FILL):
        flags = tc.fill_carry_flags(T)
        good = flags == 0
        assert good.all(axis=0).sum() == 34 and set(np.nonzero(~good.all(axis=0))[0].tolist()) == set(tc.FILL_JOINTS.values())
        assert np.nonzero(good[:, tc.FILL_JOINTS["ends"]])[0].tolist() == [0, T - 1]
        first = np.nonzero(good[:, tc.FILL_JOINTS["first_chunk"]])[0]
        assert first.max() == tc.CHUNK - 1 and len(first) == 101
        last = np.nonzero(good[:, tc.FILL_JOINTS["last_chunk"]])[0]
        assert last.min() == 2 * tc.CHUNK and len(last) == T - 2 * tc.CHUNK
        assert {1, 2, 3} == set(flags[~good].tolist())
    # the oracle on a short stand-in of the same shape of flags: the vectorised fill is the walk's
    T = 700
    X = tc.fill_carry_points()[:T]
    flags = np.zeros((T, 38), dtype=np.uint8)
    flags[1:T - 1, 3] = 1 + np.arange(T - 2) % 3
    flags[200:, 11] = 2
    flags[:500, 22] = 1
    for gap in (10, 1000000):
        assert all(np.array_equal(a, w) for a, w in zip(pr.fill_gaps(X, flags, gap), pr.fill_gaps_loop(X, flags, gap)))
