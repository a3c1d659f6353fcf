"""GPU tests of the treadmill analysis against tests/treadmill_oracle.py: tips, velocities and the slice sums bit
for bit, the integer outputs exactly, the solved quantities under their derived bars -- every stage teacher-forced on the device's own
output of the stage before --, the planted ball, two bit-equal runs inside guard words, and Core and its save on the golden recording."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402
import joint_angles_oracle as jo  # noqa: E402
import treadmill_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

W = to.HALF
FPS = 100.0
# the empty and the clipped window (1, 2, 5), a block's edge, the sum slice's edge (S samples are S / 6 frames, and S frames are six
# slices exactly), more than one slice, and the scan's second level needing a second block of block results
SIZES = (1, 2, 5, 255, 256, 257, to.S - 1, to.S, to.S + 1, 2 * to.S + 1, to.B + 1)
CENTER, RADIUS = np.array([0.4, -0.3, -4.5]), 3.0
GAIT_KEYS = ["gait_tip_position", "gait_tip_velocity", "gait_states", "gait_steps", "gait_step_metrics", "gait_phase", "gait_coupling",
             "gait_coupling_count", "gait_pattern", "gait_pattern_histogram", "gait_state_counts", "gait_thresholds", "gait_fps"]
TREADMILL_KEYS = ["treadmill_ball_center", "treadmill_ball_radius", "treadmill_ball_rms", "treadmill_ball_count", "treadmill_ball_status",
                  "treadmill_rotation", "treadmill_legs", "treadmill_residual", "treadmill_fictive", "treadmill_path", "treadmill_skipped",
                  "treadmill_params", "treadmill_fps"]
REPAIR_KEYS = ["points3d_repaired", "repair_status", "repair_counts", "repair_score", "repair_params"]


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the shared references are read-only


def _host(t):
    return t.cpu().numpy()


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _bits_where_finite(a, b):
    """NaN in the same places (a NaN's payload is not the model's) and the same bits everywhere else."""
    return _same_nan(a, b) and _bits(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


def _ratio(error, bar):
    ok = np.isfinite(bar)
    return float(np.max(error[ok] / bar[ok])) if np.any(ok) else 0.0


@functools.lru_cache(maxsize=None)
def _inputs(T):
    """(X, F, states): random poses whose tips ride near a sphere, with missing tips and one non-finite tip, a random frame and random
    states with frames of 0, 1, 2 and 6 stance legs.  Computed once per size and left unchanged."""
    rng = np.random.default_rng(T)
    X = rng.normal(0.0, 1.0, (1, 38, 3)) + 0.01 * np.cumsum(rng.normal(0.0, 1.0, (T, 38, 3)), axis=0)
    d = rng.normal(size=(T, 6, 3)) + np.array([0.0, 0.0, 2.0])   # a cap of the sphere
    angle = 0.03 * np.arange(T)   # and the cap turns, so that the tips have a velocity
    turn = to.rotation_about(np.array([0.6, 0.8, 0.0]), angle)
    d = np.einsum("tij,tlj->tli", turn, d / np.linalg.norm(d, axis=-1, keepdims=True))
    X[:, to.TIPS] = CENTER + RADIUS * d + rng.normal(0.0, 0.02, (T, 6, 3))
    if T > 6:
        X[rng.integers(0, T, size=max(T // 50, 2)), to.TIPS[1]] = 0.0
        X[T // 2, to.TIPS[3], 1] = np.inf
    F = jo.random_rotation(rng)
    states = to.random_states(T, seed=T)
    for a in (X, F, states):
        a.setflags(write=False)
    return X, F, states


def _device_tips(ops, cuda, T):
    """(tips, vel on the device, the device's own coxa medians on the host)."""
    X, F, _ = _inputs(T)
    Xd = _dev(X, cuda)
    tips, vel = ops.body_tips(Xd, FPS, _dev(F, cuda), W)
    return tips, vel, _host(ops._coxa_medians(Xd)[1])


# ------------------------------------------------------------------------------------------------------------------ every stage
@pytest.mark.parametrize("T", SIZES)
def test_every_stage_against_the_oracle(native_lib, cuda, T):
    from deepfly3d_amd import ops

    X, F, states = _inputs(T)
    tips, vel, medians = _device_tips(ops, cuda, T)
    b, v = _host(tips), _host(vel)
    want_b, want_v = to.body_tips(X, FPS, F, medians, W)
    assert _bits_where_finite(b, want_b) and _bits_where_finite(v, want_v)   # the oracle's operations one by one
    assert np.isnan(v).all() if T == 1 else np.isfinite(v).any()
    sd = _dev(states, cuda)

    # the ball, free radius: on the device's own tips
    fit = ops.fit_ball(tips, sd)
    want = to.fit_ball(b, states)
    assert _bits(_host(fit.sums), to.sums_kernel_form(b, states))   # the slice sums in the kernel's order
    assert int(fit.count) == want["count"] and int(fit.status) == want["status"]
    ball = _host(fit.ball)
    if want["status"] & to.REFUSED:
        assert np.isnan(ball[:5]).all() and not ball[5:].any()
    else:
        c_bar, r_bar = to.ball_bar(b, states, want)
        c_err, r_err = np.linalg.norm(ball[:3] - want["center"]), abs(ball[3] - want["radius"])
        m_bar = to.rms_bar(b, states, want, c_bar, r_bar)
        print(f"T = {T}: ball centre {c_err / c_bar:.2e}, radius {r_err / r_bar:.2e}, rms {abs(ball[4] - want['rms']) / m_bar:.2e} of the bar "
              f"(condition {np.linalg.cond(to.normal4(want['sums'])[0]):.0f}, {want['count']} samples)")
        assert c_err <= c_bar and r_err <= r_bar and abs(ball[4] - want["rms"]) <= m_bar

    # the ball, known radius (not at B + 1, the scan's size: the fit has no path that depends on B, and its exact sums take seconds there)
    known = ops.fit_ball(tips, sd, RADIUS)
    assert int(known.count) == want["count"]
    want_known = to.fit_ball(b, states, RADIUS) if T <= 2 * to.S + 1 else None
    if want_known is None:
        assert int(known.status) == 0 and float(known.radius) == RADIUS
    elif not want_known["status"] & to.REFUSED:
        assert int(known.status) == want_known["status"]
        k_bar = to.known_radius_bar(b, states, want_known)
        k_err = np.linalg.norm(_host(known.center) - want_known["center"])
        print(f"T = {T}: known-radius centre {k_err / k_bar:.2e} of the bar (last step {want_known['steps'][-1]:.1e})")
        assert k_err <= k_bar and float(known.radius) == RADIUS
        m_bar = to.rms_bar(b, states, want_known, k_bar, 0.0)
        assert abs(float(known.rms) - want_known["rms"]) <= m_bar
    else:
        assert int(known.status) == want_known["status"] and np.isnan(_host(known.ball)[:5]).all()

    # the rotation: on the device's own ball (the planted one where the fit was refused)
    use = fit.ball if not want["status"] & to.REFUSED else _dev(np.array([*CENTER, RADIUS, 0.0, 0.0, 0.0, 0.0]), cuda)
    c, R = _host(use)[:3], float(use[3])
    rotation, legs, residual, fictive = (_host(a) for a in ops.ball_rotation(tips, vel, sd, use))
    r = to.ball_rotation(b, v, states, c, R)
    assert legs.dtype == np.int32 and np.array_equal(legs, r["legs"])
    assert _same_nan(rotation, r["rotation"]) and _same_nan(fictive, r["fictive"]) and _same_nan(residual, r["residual"])
    ok = np.isfinite(r["bar"])
    if T >= 255:
        assert ok.sum() > T // 4 and set(np.unique(legs)) >= {0, 1, 2}   # frames of no, one and two stance legs, and solved ones
    w_err = np.linalg.norm(np.where(ok[:, None], rotation - r["rotation"], 0.0), axis=1)
    f_err = np.max(np.abs(np.where(ok[:, None], fictive - r["fictive"], 0.0)), axis=1)
    e_err = np.abs(np.where(ok, residual - r["residual"], 0.0))
    print(f"T = {T}: rotation {_ratio(w_err, r['bar']):.2e}, fictive {_ratio(f_err, r['fictive_bar']):.2e}, residual "
          f"{_ratio(e_err, r['residual_bar']):.2e} of the bar ({int(ok.sum())} frames solved)")
    assert np.all(w_err[ok] <= r["bar"][ok]) and np.all(f_err[ok] <= r["fictive_bar"][ok]) and np.all(e_err[ok] <= r["residual_bar"][ok])

    # the path: on the device's own fictive motion
    path, skipped = ops.fictive_path(_dev(fictive, cuda), FPS)
    path = _host(path)
    p = to.fictive_path(fictive, FPS)
    assert int(skipped) == p["skipped"] == int((~np.isfinite(fictive).all(axis=1)).sum())
    assert np.isfinite(path).all() and not path[0].any()
    t_err, xy_err = np.abs(path[:, 2] - p["path"][:, 2]), np.max(np.abs(path[:, :2] - p["path"][:, :2]), axis=1)
    moved = p["theta_bar"] > 0
    assert np.all(t_err[~moved] == 0.0) and np.all(xy_err[p["xy_bar"] == 0] == 0.0)
    if moved.any():
        print(f"T = {T}: theta {float(np.max(t_err[moved] / p['theta_bar'][moved])):.2e}, x and y "
              f"{float(np.max(xy_err[p['xy_bar'] > 0] / p['xy_bar'][p['xy_bar'] > 0])):.2e} of the bar")
    assert np.all(t_err <= p["theta_bar"]) and np.all(xy_err <= p["xy_bar"])


def test_edge_inputs(native_lib, cuda):
    """An all-unknown recording, a flat stance set, two legs with parallel radii, a non-finite frame, other windows."""
    from deepfly3d_amd import ops

    T = 300
    X, F, states = _inputs(T)
    tips, vel, medians = _device_tips(ops, cuda, T)
    b = _host(tips)
    # nobody is ever in stance: no samples, a refused fit, and nothing moves
    unknown = torch.full((T, 6), -1, dtype=torch.int32, device=cuda)
    fit = ops.fit_ball(tips, unknown)
    assert int(fit.count) == 0 and int(fit.status) == to.REFUSED and np.isnan(_host(fit.ball)[:5]).all() and not _host(fit.sums).any()
    rotation, legs, residual, fictive = ops.ball_rotation(tips, vel, unknown, fit)
    assert torch.isnan(rotation).all() and not legs.any() and torch.isnan(fictive).all() and torch.isnan(residual).all()
    path, skipped = ops.fictive_path(fictive, FPS)
    assert int(skipped) == T and not path.any()
    # a flat stance set: refused when the radius is free, fitted from beyond the tips when it is known
    rng = np.random.default_rng(8)
    d = rng.normal(size=(T, 6, 2))
    flat = np.empty((T, 6, 3))   # the circle in which the sphere round CENTER cuts a plane between the centre and the body's origin
    flat[..., :2] = CENTER[:2] + np.sqrt(RADIUS ** 2 - 2.0 ** 2) * d / np.linalg.norm(d, axis=-1, keepdims=True)
    flat[..., 2] = CENTER[2] + 2.0
    sd = _dev(states, cuda)
    assert int(ops.fit_ball(_dev(flat, cuda), sd).status) == to.REFUSED == to.fit_ball(flat, states)["status"]
    known, want = ops.fit_ball(_dev(flat, cuda), sd, RADIUS), to.fit_ball(flat, states, RADIUS)
    assert int(known.status) == want["status"] == to.START_BELOW
    assert np.linalg.norm(_host(known.center) - want["center"]) <= to.known_radius_bar(flat, states, want)
    assert np.linalg.norm(want["center"] - CENTER) <= 1e-9   # of the two spheres through the circle, the one beyond the tips
    # two stance legs with parallel radii leave the spin about them free: that frame is NaN, its neighbours are not
    ball = _dev(np.array([*CENTER, RADIUS, 0.0, 0.0, 0.0, 0.0]), cuda)
    two = np.ones((T, 6), dtype=np.int32)
    two[:, [0, 2]] = 0   # two legs whose tips are never missing
    par = b.copy()
    par[100, 2] = CENTER + 0.5 * (par[100, 0] - CENTER)
    got = _host(ops.ball_rotation(_dev(par, cuda), vel, _dev(two, cuda), ball)[0])
    want = to.ball_rotation(par, _host(vel), two, CENTER, RADIUS)
    assert np.isnan(got[100]).all() and np.isfinite(np.delete(got, 100, axis=0)).all() and _same_nan(got, want["rotation"])
    # a frame with a non-finite number: every tip and velocity is NaN, and the fit has no samples
    bad = np.array(F)
    bad[2, 0] = np.nan
    nt, nv = ops.body_tips(_dev(X, cuda), FPS, _dev(bad, cuda), W)
    assert torch.isnan(nt).all() and torch.isnan(nv).all() and int(ops.fit_ball(nt, sd).count) == 0
    # the widest window, clipped at both ends in every frame, and another rate
    for w, fps in ((64, 250.0), (1, 30.0)):
        gt, gv = (_host(a) for a in ops.body_tips(_dev(X, cuda), fps, _dev(F, cuda), w))
        wt, wv = to.body_tips(X, fps, F, medians, w)
        assert _bits_where_finite(gt, wt) and _bits_where_finite(gv, wv)
    # the named frame is the device's own recording frame
    named = ops.body_tips(_dev(X, cuda), FPS)
    forced = ops.body_tips(_dev(X, cuda), FPS, ops.recording_frame(_dev(X, cuda)))
    assert all(_bits(_host(a), _host(c)) for a, c in zip(named, forced))
    # min_legs
    r3 = _host(ops.ball_rotation(tips, vel, sd, ball, min_legs=3)[0])
    assert _same_nan(r3, to.ball_rotation(b, _host(vel), states, CENTER, RADIUS, min_legs=3)["rotation"])


# ------------------------------------------------------------------------------------------------------------------ the planted ball
@pytest.mark.parametrize("kind", ["walk", "yaw"])
def test_planted_ball(native_lib, cuda, golden_dir, kind):
    from deepfly3d_amd import ops

    planted = to.planted_ball(go.planted_pose(golden_dir), kind)
    r = ops.treadmill(_dev(planted["X"], cuda), to.PLANTED["fps"], states=_dev(planted["states"], cuda))   # the recording frame
    assert r.fps == to.PLANTED["fps"] and r.params[3:] == (W, to.MIN_LEGS, to.ITERATIONS) and np.isnan(r.params[:3]).all()
    found = dict(fit=dict(center=_host(r.ball.center), radius=float(r.ball.radius), rms=float(r.ball.rms), count=int(r.ball.count),
                          status=int(r.ball.status)),
                 rotation=_host(r.rotation), legs=_host(r.legs), fictive=_host(r.fictive), path=_host(r.path))
    worst, bound = to.check_planted(found, planted, kind)
    print(f"{kind}: rotation off by {worst:.3e} relative, chord bound {bound:.3e}")
    assert int(r.skipped) == int((~np.isfinite(found["fictive"]).all(axis=1)).sum())
    if kind == "walk":   # gait's own states: every tip is on the sphere whatever its state, and a known radius changes nothing
        own = ops.treadmill(_dev(planted["X"], cuda), to.PLANTED["fps"], radius=planted["radius"])
        assert own.params[:3] == (planted["radius"], go.ON, go.OFF) and int(own.ball.status) == 0
        assert np.all(_host(own.states)[planted["states"] == 0] == 0)
        assert np.linalg.norm(_host(own.ball.center) - planted["center"]) <= 1e-9 and float(own.ball.radius) == planted["radius"]


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_determinism_guard_words_and_a_side_stream(native_lib, cuda):
    """The raw entries on sentinel-filled buffers inside guard words, the workspace too, on a stream of their own: two runs are
    bit-equal, every output element is written and nothing outside is."""
    lib = native_lib
    T = 2 * to.S // 6 + 300   # three sum slices, four scan blocks
    X, F, states = _inputs(300)
    rng = np.random.default_rng(5)
    X = np.concatenate([X, X[::-1], X, X])[:T] + rng.normal(0.0, 0.01, (T, 38, 3))
    states = to.random_states(T, seed=9)
    GUARD = 64
    need = lib.df3d_ball_work_bytes(T)
    assert need % 16 == 0
    side = torch.cuda.Stream(device=cuda)
    st = side.cuda_stream
    fills = {torch.float64: -1.2345e30, torch.int32: -77, torch.int64: -7777}

    def guarded(count, dtype=torch.float64):
        t = torch.full((count + 2 * GUARD,), fills[dtype], dtype=dtype, device=cuda)
        return t, t.data_ptr() + GUARD * t.element_size()

    def inner(t):
        a = t.cpu().numpy()
        fill = fills[t.dtype]
        assert np.all(a[:GUARD] == fill) and np.all(a[-GUARD:] == fill), "a guard word was written"
        return a[GUARD:-GUARD]

    from deepfly3d_amd import ops

    runs = []
    with torch.cuda.stream(side):
        Xd, Fd, sd = _dev(X, cuda), _dev(F, cuda), _dev(states, cuda)
        coxa = ops._coxa_medians(Xd)[1].contiguous()
        for _ in range(2):
            tip, vel = guarded(T * 18), guarded(T * 18)
            ball, info, sums = guarded(8), guarded(2, torch.int64), guarded(17)
            omega, legs, residual, fictive = guarded(T * 3), guarded(T, torch.int32), guarded(T), guarded(T * 3)
            path, skipped = guarded(T * 3), guarded(1, torch.int64)
            work = guarded(need // 8)
            for rc in (lib.df3d_ball_tips(Xd.data_ptr(), T, Fd.data_ptr(), coxa.data_ptr(), FPS, W, tip[1], vel[1], st),
                       lib.df3d_ball_fit(tip[1], sd.data_ptr(), T, 1, RADIUS, 8, to.PIVOT_MIN, ball[1], info[1], sums[1], work[1], need, st),
                       lib.df3d_ball_rotation(tip[1], vel[1], sd.data_ptr(), T, ball[1], 2, to.FRAME_PIVOT_MIN, omega[1], legs[1], residual[1],
                                              fictive[1], st),
                       lib.df3d_ball_path(fictive[1], T, FPS, path[1], skipped[1], work[1], need, st)):
                assert rc == 0, lib.df3d_last_error()
            side.synchronize()
            inner(work[0])
            runs.append({k: inner(v[0]).copy() for k, v in dict(tip=tip, vel=vel, ball=ball, info=info, sums=sums, omega=omega, legs=legs,
                                                                residual=residual, fictive=fictive, path=path, skipped=skipped).items()})
    first, second = runs
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), f"{k} differs between two runs"
        assert not np.any(first[k] == fills[torch.from_numpy(first[k]).dtype]), f"{k} was not written everywhere"
    b = first["tip"].reshape(T, 6, 3)
    assert _bits(first["sums"], to.sums_kernel_form(b, states)) and first["info"].tolist() == [int(to.samples(b, states).sum()), 0]
    want = to.fit_ball(b, states, RADIUS)
    assert np.linalg.norm(first["ball"][:3] - want["center"]) <= to.known_radius_bar(b, states, want)
    assert np.isfinite(first["omega"]).any() and first["skipped"][0] == (~np.isfinite(first["fictive"].reshape(T, 3)).all(axis=1)).sum()


def test_on_non_contiguous_and_empty_input(native_lib, cuda):
    from deepfly3d_amd import ops

    X, F, states = _inputs(300)
    sd = _dev(states, cuda)
    plain = ops.treadmill(_dev(X, cuda), FPS, _dev(F, cuda), states=sd)
    wide = _dev(np.repeat(X, 2, axis=2), cuda)[:, :, ::2]   # not contiguous: ops copies
    states2 = torch.stack((sd, sd), dim=2)[:, :, 1]
    assert not wide.is_contiguous() and not states2.is_contiguous()
    again = ops.treadmill(wide, FPS, np.array(F), states=states2)
    for name in ("tip", "vel", "rotation", "legs", "residual", "fictive", "path"):
        assert _bits(_host(getattr(plain, name)), _host(getattr(again, name))), name
    assert _bits(_host(plain.ball.ball), _host(again.ball.ball)) and int(plain.skipped) == int(again.skipped)
    empty = ops.treadmill(torch.zeros((0, 38, 3), dtype=torch.float64, device=cuda), FPS)
    assert empty.tip.shape == (0, 6, 3) and empty.states.shape == (0, 6) and empty.rotation.shape == (0, 3) and empty.path.shape == (0, 3)
    assert int(empty.ball.count) == 0 and int(empty.ball.status) == to.REFUSED and torch.isnan(empty.ball.center).all() and int(empty.skipped) == 0
    with pytest.raises(ValueError, match="states must hold the 300 frames"):
        ops.treadmill(_dev(X, cuda), FPS, states=sd[:10])
    with pytest.raises(ValueError, match='body_frame must be "recording" or a'):
        ops.body_tips(_dev(X, cuda), FPS, "per_frame")
    with pytest.raises(ValueError, match=r"an explicit body_frame must be \[3, 3\]"):
        ops.body_tips(_dev(X, cuda), FPS, np.zeros((300, 3, 3)))
    with pytest.raises(ValueError, match="ball must be a BallFit"):
        ops.ball_rotation(plain.tip, plain.vel, sd, plain.ball.ball[:5])


# ------------------------------------------------------------------------------------------------------------------ Core and its save
def _recording(tmp_path, golden_dir):
    """(folder, result pickle): 15 frames (links to the sample's frame 0) and an earlier result holding the golden detections and cameras."""
    folder = tmp_path / "working"
    folder.mkdir()
    for c in range(7):
        for t in range(15):
            os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
    folder = str(folder)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    os.makedirs(folder + "_df3d")
    pkl = os.path.join(folder + "_df3d", "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
    res = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "distort": g3["distort"][c], "intr": g3["intr"][c]} for c in range(7)}
    res.update(points2d=g3["points2d"], camera_ordering=g3["camera_ordering"], heatmap_confidence=g3["heatmap_confidence"])
    with open(pkl, "wb") as f:
        pickle.dump(res, f)
    return folder, pkl


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_core_treadmill_and_save(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))

    def saved(**flags):
        core.save(**flags)
        with open(pkl, "rb") as f:
            return f.read()

    plain = saved()
    before = pickle.loads(plain)
    T = 15
    r = core.treadmill(on=0.5, off=-0.5, radius=4.0)
    assert isinstance(r, ops.TreadmillResult) and r.fps == cfg.SPECTROGRAM_FPS and r.params == (4.0, 0.5, -0.5, cfg.GAIT_DIFF_HALF, 2, 8)
    assert all(isinstance(a, np.ndarray) for a in (r.tip, r.vel, r.states, r.rotation, r.legs, r.residual, r.fictive, r.path, r.ball.ball))
    assert isinstance(r.skipped, int) and r.tip.shape == (T, 6, 3) and r.path.shape == (T, 3) and r.legs.dtype == np.int32
    # against the oracle in the device's own recording frame, on the device's own tips
    X = np.ascontiguousarray(core.camNet.points3d, dtype=np.float64)
    Xd = _dev(X, cuda)
    F, medians = _host(ops.recording_frame(Xd))[0], _host(ops._coxa_medians(Xd)[1])
    want_b, want_v = to.body_tips(X, r.fps, F, medians)
    assert _bits_where_finite(r.tip, want_b) and _bits_where_finite(r.vel, want_v)
    assert np.array_equal(r.states, go.states_of(r.vel[..., 0], 0.5, -0.5))
    want = to.fit_ball(r.tip, r.states, 4.0)
    assert int(r.ball.count) == want["count"] and int(r.ball.status) == want["status"]
    assert _same_nan(r.rotation, to.ball_rotation(r.tip, r.vel, r.states, r.ball.center, float(r.ball.radius))["rotation"])

    assert saved() == plain   # without the flag: the bytes written before
    run = pickle.loads(saved(treadmill=True))
    assert list(run.keys()) == list(before.keys()) + TREADMILL_KEYS and all(_same(before[k], run[k]) for k in before)
    k = {name[len("treadmill_"):]: run[name] for name in TREADMILL_KEYS}
    assert k["ball_center"].shape == (3,) and isinstance(k["ball_radius"], float) and isinstance(k["ball_rms"], float)
    assert isinstance(k["ball_count"], int) and isinstance(k["ball_status"], int) and isinstance(k["skipped"], int) and isinstance(k["fps"], float)
    assert k["rotation"].shape == (T, 3) and k["legs"].shape == (T,) and k["legs"].dtype == np.int32 and k["residual"].shape == (T,)
    assert k["fictive"].shape == (T, 3) and k["path"].shape == (T, 3) and k["params"].dtype == np.float64
    assert np.isnan(k["params"][0]) and k["params"][1:].tolist() == [cfg.GAIT_SWING_ON, cfg.GAIT_SWING_OFF, cfg.GAIT_DIFF_HALF, 2, 8]
    direct = core.treadmill()
    assert _same(k["rotation"], direct.rotation) and _same(k["path"], direct.path) and k["skipped"] == direct.skipped
    assert _same(k["ball_center"], direct.ball.center) and k["skipped"] == to.fictive_path(k["fictive"], k["fps"])["skipped"]
    known = pickle.loads(saved(treadmill=True, ball_radius=4.0))
    assert known["treadmill_ball_radius"] == 4.0 or known["treadmill_ball_status"] & to.REFUSED
    assert known["treadmill_params"][0] == 4.0 and list(known.keys()) == list(run.keys())

    # with gait and the repair: the gait keys, then the treadmill keys, then the repair keys; the states are computed once per pose
    calls = []
    counted = ops.gait_states
    monkeypatch.setattr(ops, "gait_states", lambda *a, **kw: calls.append(1) or counted(*a, **kw))
    both = pickle.loads(saved(gait=True, treadmill=True, gait_on=0.5, gait_off=-0.5))
    assert len(calls) == 1
    assert list(both.keys()) == list(before.keys()) + GAIT_KEYS + TREADMILL_KEYS
    assert both["treadmill_params"][1:3].tolist() == [0.5, -0.5]   # the thresholds behind the shared states
    again = core.treadmill(on=0.5, off=-0.5)
    assert _same(both["treadmill_rotation"], again.rotation) and _same(both["treadmill_path"], again.path)
    del calls[:]
    full = pickle.loads(saved(gait=True, treadmill=True, repair_pose=True))
    assert len(calls) == 1 and list(full.keys()) == list(before.keys()) + GAIT_KEYS + TREADMILL_KEYS + REPAIR_KEYS
    repaired = core.treadmill(repair=True)
    assert _same(full["treadmill_path"], repaired.path) and _same(full["treadmill_legs"], repaired.legs)
    assert saved() == plain
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_treadmill(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    with open(pkl, "rb") as f:
        earlier = f.read()
    order = [str(c) for c in range(7)]

    def reopen(*flags):
        with open(pkl, "wb") as f:
            f.write(earlier)
        assert cli.main([folder, "--skip-pose-estimation", *flags, "--order"] + order) == 0
        with open(pkl, "rb") as f:
            return pickle.load(f)

    before = reopen("--joint-angles")
    run = reopen("--joint-angles", "--treadmill", "--ball-radius", "4")
    assert list(run.keys()) == list(before.keys()) + TREADMILL_KEYS and all(_same(before[k], run[k]) for k in before)
    assert run["treadmill_params"][0] == 4.0
    alone = reopen("--treadmill")
    assert list(alone.keys()) == [k for k in before if k not in ("joint_angles", "segment_lengths")] + TREADMILL_KEYS
    with open(pkl, "wb") as f:
        f.write(earlier)
    with pytest.raises(SystemExit):
        cli.main([folder, "--skip-pose-estimation", "--ball-radius", "3", "--order"] + order)
    with open(pkl, "rb") as f:
        assert f.read() == earlier   # refused before any work: the earlier result is untouched
    config.pop("image_shape", None)
