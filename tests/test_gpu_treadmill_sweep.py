"""GPU sweep of the treadmill fit (csrc/treadmill.hip, DESIGN.md section 21, "swept") on the families of tests/treadmill_cases.py, which
tests/test_treadmill_cases_host.py certifies on the CPU: every Gauss-Newton step teacher-forced on the device's own centre before it
(a converged comparison sees the right-hand side alone: the fixed point of c <- c + N^-1 g is g = 0 whatever N), every path of the
status word on purpose, the rotation's and the path's edge inputs, and the blocked scans of treadmill.hip, gait.hip and
pose_repair.hip at three chunks of block results, where the carry is used a second time.  Every test prints the largest fraction of
its bar that it used."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402
import pose_repair_oracle as pr  # noqa: E402
import treadmill_cases as tc  # noqa: E402
import treadmill_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

FPS = tc.FPS
STEPS = tuple(range(1, 7)) + (63, 64)      # c_1 .. c_6 each against the step from the one before, and c_64 against the step from c_63


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the shared cases are read-only


def _host(t):
    return t.cpu().numpy()


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def _refused(fit):
    ball = _host(fit.ball)
    return np.isnan(ball[:5]).all() and _bits(ball[5:], np.zeros(3))


# ------------------------------------------------------------------------------------------------------------------ teacher-forced steps
@pytest.mark.parametrize("name", tc.FAR_START)
def test_every_gauss_newton_step_against_the_oracles_from_the_same_centre(native_lib, cuda, name):
    from deepfly3d_amd import ops

    case = tc.fit_case(name)
    b, states, R = case
    bd, sd = _dev(b, cuda), _dev(states, cuda)
    free = ops.fit_ball(bd, sd)
    sums = _host(free.sums)
    assert _bits(sums, to.sums_kernel_form(b, states))
    if int(free.status) & to.REFUSED:      # no algebraic centre: the start beyond the mean, on the device's own sums
        start, status = to.start_below(sums, R), to.START_BELOW
    else:                                  # the algebraic kernel is the same with a known radius, and so are its bits
        start, status = _host(free.center), 0
    assert status == to.fit_ball(b, states, R)["status"]
    centres = {0: start}
    worst = rms_worst = 0.0
    for k in STEPS:
        fit = ops.fit_ball(bd, sd, R, iterations=k)
        assert int(fit.status) == status and int(fit.count) == int(sums[0]) and _bits(_host(fit.sums), sums)
        assert _bits(_host(fit.radius), np.float64(R)) and not _host(fit.ball)[5:].any()
        centres[k] = c = _host(fit.center)
        # rms: the oracle's at the device's own final centre
        mine = dict(center=c, radius=R, count=int(sums[0]), rms=float(np.sqrt(to.step_sums(b, states, c, R)[9] / sums[0])))
        m_bar = to.rms_bar(b, states, mine, 0.0, 0.0)
        rms_worst = max(rms_worst, abs(float(fit.rms) - mine["rms"]) / m_bar)
        assert abs(float(fit.rms) - mine["rms"]) <= m_bar
        if k - 1 not in centres:
            continue
        before = centres[k - 1]
        want, _ = to.gauss_newton_step(b, states, before, R)
        bar = to.step_bar(b, states, before, R)
        err = float(np.linalg.norm(c - want))
        print(f"{name} step {k}: length {np.linalg.norm(want - before):.3g}, off by {err:.3g}, {err / bar:.2e} of the bar {bar:.3g}")
        worst = max(worst, err / bar)
        assert err <= bar, (name, k, err, bar)
    # 64 steps: the oracle's fixed point
    want = to.fit_ball(b, states, R, 64)
    k_bar = to.known_radius_bar(b, states, want)
    k_err = float(np.linalg.norm(centres[64] - want["center"]))
    print(f"{name}: the largest step error is {worst:.2e} of step_bar, rms {rms_worst:.2e} of rms_bar, the centre after 64 steps "
          f"{k_err / k_bar:.2e} of known_radius_bar (the oracle's last step {want['steps'][-1]:.1e})")
    assert want["status"] == status and k_err <= k_bar


# ------------------------------------------------------------------------------------------------------------------ counts, degenerate
@pytest.mark.parametrize("name", tc.COUNTS + tc.DEGENERATE)
def test_status_paths(native_lib, cuda, name):
    from deepfly3d_amd import ops

    case = tc.fit_case(name)
    b, states, R = case
    bd, sd = _dev(b, cuda), _dev(states, cuda)
    # a velocity for the rotation on the fit: any finite one
    vd = _dev(np.random.default_rng(3).normal(size=b.shape), cuda)
    used = {}
    for radius in (None, R):
        fit, want = ops.fit_ball(bd, sd, radius), to.fit_ball(b, states, radius)
        label = "free" if radius is None else "known"
        assert int(fit.status) == want["status"] and int(fit.count) == want["count"], (name, label, int(fit.status), int(fit.count))
        assert _bits(_host(fit.sums), to.sums_kernel_form(b, states))
        rotation, legs, residual, fictive = (_host(a) for a in ops.ball_rotation(bd, vd, sd, fit))
        assert np.array_equal(legs, to.samples(b, states).sum(axis=1).astype(np.int32)) and legs.dtype == np.int32
        if want["status"] & to.REFUSED:
            assert _refused(fit)
            assert np.isnan(rotation).all() and np.isnan(residual).all() and np.isnan(fictive).all()
            continue
        c, rms = _host(fit.center), float(fit.rms)
        if radius is None:
            c_bar, r_bar = to.ball_bar(b, states, want)
            r_err = abs(float(fit.radius) - want["radius"])
            used[f"{label} radius"] = r_err / r_bar
            assert r_err <= r_bar
        else:
            c_bar, r_bar = to.known_radius_bar(b, states, want), 0.0
            assert _bits(_host(fit.radius), np.float64(R))
        c_err, m_bar = float(np.linalg.norm(c - want["center"])), to.rms_bar(b, states, want, c_bar, r_bar)
        used[f"{label} centre"], used[f"{label} rms"] = c_err / c_bar, abs(rms - want["rms"]) / m_bar
        assert c_err <= c_bar and abs(rms - want["rms"]) <= m_bar and not _host(fit.ball)[5:].any()
        if name in ("n4", "spread4") and radius is None:      # four samples on a sphere: the planted one, and no residual beyond the bar
            assert np.linalg.norm(c - tc.CENTER) <= c_bar + 1e-12 and abs(float(fit.radius) - tc.RADIUS) <= r_bar + 1e-12 and rms <= m_bar
    print(f"{name}: " + (", ".join(f"{k} {v:.2e}" for k, v in used.items()) + " of the bar" if used else "refused both ways"))


# ------------------------------------------------------------------------------------------------------------------ the rotation
def test_rotation_cases(native_lib, cuda):
    from deepfly3d_amd import ops

    b, v, states, usable = tc.rotation_case()
    bd, vd, sd = _dev(b, cuda), _dev(v, cuda), _dev(states, cuda)
    worst = dict(rotation=0.0, fictive=0.0, residual=0.0)
    for ball_name, ball in tc.ROTATION_BALLS.items():
        ball_d = _dev(np.array([*ball, 0.0, 0.0, 0.0, 0.0]), cuda)
        for min_legs in range(2, 7):
            rotation, legs, residual, fictive = (_host(a) for a in ops.ball_rotation(bd, vd, sd, ball_d, min_legs=min_legs))
            r = to.ball_rotation(b, v, states, np.array(ball[:3]), ball[3], min_legs)
            assert legs.dtype == np.int32 and np.array_equal(legs, r["legs"]) and np.array_equal(legs, usable)
            assert _same_nan(rotation, r["rotation"]) and _same_nan(residual, r["residual"]) and _same_nan(fictive, r["fictive"]), (ball_name, min_legs)
            ok = np.isfinite(r["bar"])
            assert np.array_equal(ok, np.isfinite(rotation).all(axis=1))
            if ball_name in ("nan_radius", "inf_radius"):
                assert not ok.any() and np.isnan(rotation).all() and np.isnan(fictive).all()
                continue
            if ball_name == "planted":
                assert ok.sum() == (usable >= min_legs).sum() - (min_legs <= 3)      # but for the frame of parallel radii
            w_err = np.linalg.norm(rotation[ok] - r["rotation"][ok], axis=1)
            e_err = np.abs(residual[ok] - r["residual"][ok])
            worst["rotation"] = max(worst["rotation"], float(np.max(w_err / r["bar"][ok])))
            worst["residual"] = max(worst["residual"], float(np.max(e_err / r["residual_bar"][ok])))
            assert np.all(w_err <= r["bar"][ok]) and np.all(e_err <= r["residual_bar"][ok])
            if ball_name == "origin":      # no direction from the ball to the fly: the rotation is solved, nothing moves
                assert np.isnan(fictive).all() and ok.any()
                path, skipped = ops.fictive_path(_dev(fictive, cuda), FPS)
                assert int(skipped) == len(b) and _bits(_host(path), np.zeros((len(b), 3)))
            else:
                f_err = np.max(np.abs(fictive[ok] - r["fictive"][ok]), axis=1)
                worst["fictive"] = max(worst["fictive"], float(np.max(f_err / r["fictive_bar"][ok])))
                assert np.all(f_err <= r["fictive_bar"][ok])
    print("rotation cases: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + " of the bar")


# ------------------------------------------------------------------------------------------------------------------ the path
def _check_path(ops, cuda, f):
    """The device's path of f against the oracle's; returns (theta, xy: the largest fractions of their bars, device seconds)."""
    fd = _dev(f, cuda)
    torch.cuda.synchronize(cuda)
    t0 = time.perf_counter()
    path, skipped = ops.fictive_path(fd, FPS)
    torch.cuda.synchronize(cuda)
    seconds = time.perf_counter() - t0
    path = _host(path)
    p = to.fictive_path(f, FPS)
    moves = np.isfinite(f).all(axis=1)
    assert int(skipped) == p["skipped"] == int((~moves).sum())
    assert np.isfinite(path).all()
    first = int(np.argmax(moves)) if moves.any() else len(f) - 1
    assert _bits(path[:first + 1], np.zeros((first + 1, 3)))      # nothing has moved yet: +0.0, bit for bit
    t_err, xy_err = np.abs(path[:, 2] - p["path"][:, 2]), np.max(np.abs(path[:, :2] - p["path"][:, :2]), axis=1)
    assert np.all(t_err <= p["theta_bar"]) and np.all(xy_err <= p["xy_bar"])
    tb, xb = p["theta_bar"] > 0, p["xy_bar"] > 0
    return (float(np.max(t_err[tb] / p["theta_bar"][tb])) if tb.any() else 0.0, float(np.max(xy_err[xb] / p["xy_bar"][xb])) if xb.any() else 0.0,
            seconds, path, p)


@pytest.mark.parametrize("name", [n for n in tc.PATHS if n != "carry3"])
def test_path_cases(native_lib, cuda, name):
    from deepfly3d_amd import ops

    f = tc.path_case(name)
    theta, xy, _, path, p = _check_path(ops, cuda, f)
    if name == "edges":
        assert p["skipped"] == sum(b - a for a, b in tc.PATH_EDGE_RUNS) + 3
    if name == "large_yaw":
        assert path[-1, 2] > 1e5
    print(f"path {name}: theta {theta:.2e}, x and y {xy:.2e} of the bar")


# ------------------------------------------------------------------------------------------------------------------ three chunks of carry
def test_three_chunks_of_carry_path(native_lib, cuda):
    """path_carry_kernel: the third chunk's only entry is the first chunk's total, carried over a second chunk that adds nothing."""
    from deepfly3d_amd import ops

    f = tc.path_case("carry3")
    theta, xy, seconds, path, p = _check_path(ops, cuda, f)
    assert p["path"][-1].all() and _bits(path[tc.CHUNK:-1], np.repeat(path[tc.CHUNK:tc.CHUNK + 1], tc.T3 - 1 - tc.CHUNK, axis=0))
    assert abs(path[-1, 2] - p["path"][-1, 2]) <= p["theta_bar"][-1] and p["theta_bar"][-1] < 1e-6 * abs(p["path"][-1, 2])   # (a lost chunk is not within this)
    print(f"three chunks, fictive_path at T = {tc.T3}: theta {theta:.2e}, x and y {xy:.2e} of the bar, {seconds * 1e3:.2f} ms on the device")


def test_three_chunks_of_carry_gait_states(native_lib, cuda):
    """gait_scan_carry_kernel: every leg's only decisive sample lies in the first chunk, and every later state is still that one."""
    from deepfly3d_amd import ops

    vel = tc.gait_carry_velocity(go.ON, go.OFF)
    vd = _dev(vel, cuda)
    torch.cuda.synchronize(cuda)
    t0 = time.perf_counter()
    states = ops.gait_states(vd, go.ON, go.OFF)
    torch.cuda.synchronize(cuda)
    seconds = time.perf_counter() - t0
    states = _host(states)
    want = go.states_of(vel[..., 0], go.ON, go.OFF)
    assert states.dtype == np.int32 and _bits(states, want)
    code = {"swing": 1, "stance": 0, "nan": -1}
    for leg, t, what in tc.GAIT_DECISIVE:
        assert (states[:t, leg] == -1).all() and (states[t:, leg] == code[what]).all()
    print(f"three chunks, gait_states at T = {tc.T3}: exact, {seconds * 1e3:.2f} ms on the device")


@pytest.mark.parametrize("T", [tc.T3, tc.T3_FILL])
def test_three_chunks_of_carry_fill_gaps(native_lib, cuda, T):
    """repair_scan_carry_kernel, forwards and on the reversed index.  At T3_FILL the third chunk holds frames that are interpolated
    from a good frame of the first chunk (tests/treadmill_cases.py says why T3 alone cannot show a carry that forgot it)."""
    from deepfly3d_amd import ops

    X, flags = tc.fill_carry_points()[:T], tc.fill_carry_flags(T)
    Xd, fd = _dev(X, cuda), _dev(flags, cuda)
    for gap in (1000000, 10):
        torch.cuda.synchronize(cuda)
        t0 = time.perf_counter()
        got = ops.fill_gaps(Xd, fd, gap)
        torch.cuda.synchronize(cuda)
        seconds = time.perf_counter() - t0
        want = pr.fill_gaps(X, flags, gap)
        assert all(_bits(_host(g), w) for g, w in zip(got, want)), gap
        status = want[1]
        ends = status[1:T - 1, tc.FILL_JOINTS["ends"]]
        assert np.isin(ends, (pr.MISSING_FILLED, pr.OUTLIER_FILLED) if gap > 10 else (pr.MISSING_LEFT, pr.OUTLIER_REMOVED)).all()
        print(f"three chunks, fill_gaps at T = {T}, max_gap {gap}: bit for bit, {seconds * 1e3:.2f} ms on the device")
        del got
