"""GPU tests of the gait analysis against tests/gait_oracle.py: tip and velocity under the derived bar, the
integer outputs and the phase exactly -- teacher-forced on the device's own floats --, the coupling under its bar, the planted walker,
two bit-equal runs inside guard words, and Core and the command line on the golden recording."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402

pytestmark = pytest.mark.gpu

W = go.HALF
# window clipping (1, 2, 3, 2 w, 2 w + 1), a block's edge, the coupling slice's edge, more than 256 blocks per leg (the scan's carry)
SIZES = (1, 2, 3, 2 * W, 2 * W + 1, 255, 256, 257, 2047, 2048, 2049, 65537)
FPS = 100.0
GAIT_KEYS = ["gait_tip_position", "gait_tip_velocity", "gait_states", "gait_steps", "gait_step_metrics", "gait_phase", "gait_coupling",
             "gait_coupling_count", "gait_pattern", "gait_pattern_histogram", "gait_state_counts", "gait_thresholds", "gait_fps"]


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the shared references are read-only


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _bits_where_finite(a, b):
    """NaN in the same places (a NaN's payload is not the model's) and the same bits everywhere else."""
    return _same_nan(a, b) and _bits(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


@functools.lru_cache(maxsize=None)
def _poses(T):
    """(X, F, oracle tip, oracle vel, bar): computed once per size and left unchanged."""
    X = go.random_poses(T, seed=T)
    F = go.random_frames(T, seed=T) if T % 2 else go.random_frames(1, seed=T)[0]   # a frame per pose, or one for all
    tip, vel = go.tip_kinematics(X, FPS, F, W)
    out = (X, F, tip, vel, go.velocity_bar(X, FPS, F, W))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _series(T):
    """(vel [T, 6, 3] whose anterior component is gait_oracle.u_cases, a tip [T, 6, 3], the oracle's states of it)."""
    rng = np.random.default_rng(1000 + T)
    vel = rng.normal(size=(T, 6, 3))
    vel[..., 0] = go.u_cases(T, seed=T)
    tip = rng.normal(size=(T, 6, 3))
    tip[rng.random((T, 6)) < 0.01] = np.nan
    states = go.states_of(vel[..., 0])
    for a in (vel, tip, states):
        a.setflags(write=False)
    return vel, tip, states


# ------------------------------------------------------------------------------------------------------------------ tip and velocity
@pytest.mark.parametrize("T", SIZES)
def test_tip_and_velocity_against_the_oracle(native_lib, cuda, T):
    from deepfly3d_amd import ops

    X, F, want_tip, want_vel, bar = _poses(T)
    tip, vel = (a.cpu().numpy() for a in ops.tip_kinematics(_dev(X, cuda), FPS, _dev(F, cuda), W))
    assert _same_nan(tip, want_tip) and _same_nan(vel, want_vel)
    assert np.isnan(vel).all() if T == 1 else np.isfinite(vel).any()
    ok = np.isfinite(want_vel)
    fraction = float(np.max(np.abs(vel - want_vel)[ok] / bar[ok])) if ok.any() else 0.0
    print(f"T = {T}: velocity {fraction:.3f} of the bar")
    assert np.all(np.abs(vel - want_vel)[ok] <= bar[ok])
    # the tip has the velocity's form with d = P4 - P0 and no scale: the same bar without fps / (b - a)
    with np.errstate(invalid="ignore"):
        d = np.abs(X[:, go.TIPS] - X[:, go.COXAE])
    tip_bar = 8.0 * go.U * np.einsum("trk,tlk->tlr", np.abs(np.broadcast_to(F, (T, 3, 3))), d)
    ok = np.isfinite(want_tip)
    assert np.all(np.abs(tip - want_tip)[ok] <= tip_bar[ok])


def test_velocity_windows_frames_and_defaults(native_lib, cuda):
    from deepfly3d_amd import ops

    T = 100
    X = go.random_poses(T, seed=7)
    Xd = _dev(X, cuda)
    for w in (1, 7, 64):   # 64: clipped at both ends in every frame
        F = go.random_frames(T, seed=w)
        tip, vel = (a.cpu().numpy() for a in ops.tip_kinematics(Xd, 250.0, _dev(F, cuda), w))
        want_tip, want_vel = go.tip_kinematics(X, 250.0, F, w)
        bar = go.velocity_bar(X, 250.0, F, w)
        ok = np.isfinite(want_vel)
        assert _same_nan(vel, want_vel) and np.all(np.abs(vel - want_vel)[ok] <= bar[ok]) and _same_nan(tip, want_tip)
    # the named frames are the device's own (ops.recording_frame, ops.body_frame): teacher-forced on them
    for name, frames in (("recording", ops.recording_frame(Xd)), ("per_frame", ops.body_frame(Xd))):
        got = ops.tip_kinematics(Xd, FPS, name)
        forced = ops.tip_kinematics(Xd, FPS, frames)
        assert all(_bits(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(got, forced))
        want_tip, want_vel = go.tip_kinematics(X, FPS, frames.cpu().numpy().reshape(-1, 3, 3) if name == "per_frame" else frames.cpu().numpy()[0])
        vel = got[1].cpu().numpy()
        ok = np.isfinite(want_vel)
        bar = go.velocity_bar(X, FPS, frames.cpu().numpy().reshape(-1, 3, 3) if name == "per_frame" else frames.cpu().numpy()[0])
        assert _same_nan(vel, want_vel) and np.all(np.abs(vel - want_vel)[ok] <= bar[ok])
    # a frame with a non-finite number: tip and velocity of that pose are NaN
    F = go.random_frames(T, seed=3)
    F[11, 2, 0] = np.nan
    tip, vel = (a.cpu().numpy() for a in ops.tip_kinematics(Xd, FPS, _dev(F, cuda)))
    want_tip, want_vel = go.tip_kinematics(X, FPS, F)
    assert np.isnan(tip[11]).all() and np.isnan(vel[11]).all() and _same_nan(tip, want_tip) and _same_nan(vel, want_vel)


# ------------------------------------------------------------------------------------------------------------------ the chain, exactly
@pytest.mark.parametrize("T", SIZES)
def test_states_steps_phase_patterns_exactly(native_lib, cuda, T):
    """Random u with long in-band runs across block edges, runs of NaN, a decisive sample as the last lane of a block and the first
    of the next, a leg that never leaves the band and one that alternates every frame (gait_oracle.u_cases)."""
    from deepfly3d_amd import ops

    vel, tip, want_states = _series(T)
    vd, td = _dev(vel, cuda), _dev(tip, cuda)
    states = ops.gait_states(vd)
    got = states.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want_states)
    steps, metrics = (a.cpu().numpy() for a in ops.gait_steps(states, td, FPS))
    want_steps, want_metrics = go.steps_of(want_states, tip, FPS)
    assert steps.dtype == np.int64 and np.array_equal(steps, want_steps) and metrics.shape == want_metrics.shape
    assert _bits_where_finite(metrics[:, 2], want_metrics[:, 2])   # the stride: the same difference of the same two tips
    bar = go.duration_bar(want_metrics[:, :2])
    assert np.all(np.abs(metrics[:, :2] - want_metrics[:, :2]) <= bar)
    if len(steps):
        print(f"T = {T}: {len(steps)} steps, durations {float(np.max(np.abs(metrics[:, :2] - want_metrics[:, :2]) / bar)):.3f} of the bar")
    phase = ops.gait_phase(states)
    assert _bits(phase.cpu().numpy(), go.phase_of(want_states))
    for g, w in zip(ops.gait_patterns(states), go.patterns(want_states)):
        assert _bits(g.cpu().numpy(), w)
    # the coupling of the device's own phase
    mean, count = (a.cpu().numpy() for a in ops.gait_coupling(phase))
    want_mean, want_count = go.coupling(phase.cpu().numpy())
    assert count.dtype == np.int64 and np.array_equal(count, want_count) and _same_nan(mean, want_mean)
    bar = go.coupling_bar(want_count)[..., None] * np.ones(2)
    ok = np.isfinite(want_mean)
    if ok.any():
        print(f"T = {T}: coupling {float(np.max(np.abs(mean - want_mean)[ok] / bar[ok])):.2e} of the bar")
    assert np.all(np.abs(mean - want_mean)[ok] <= bar[ok])


def test_other_thresholds_and_a_dense_coupling(native_lib, cuda):
    """Thresholds other than the defaults, and phases that are finite nearly everywhere: every pair of legs meets in every slice."""
    from deepfly3d_amd import ops

    T = 5000
    rng = np.random.default_rng(11)
    vel = rng.normal(size=(T, 6, 3))
    vel[..., 0] = np.sin(np.arange(T)[:, None] * (2 * np.pi / rng.uniform(13.0, 40.0, 6)) + rng.uniform(0, 6, 6)) + 0.05 * rng.normal(size=(T, 6))
    vel[rng.integers(0, T, 5), rng.integers(0, 6, 5), 0] = np.nan
    want = go.states_of(vel[..., 0], 0.5, -0.25)
    states = ops.gait_states(_dev(vel, cuda), 0.5, -0.25)
    assert np.array_equal(states.cpu().numpy(), want)
    phase = ops.gait_phase(states)
    assert _bits(phase.cpu().numpy(), go.phase_of(want)) and np.isfinite(phase.cpu().numpy()).mean() > 0.9
    mean, count = (a.cpu().numpy() for a in ops.gait_coupling(phase))
    want_mean, want_count = go.coupling(phase.cpu().numpy())
    bar = go.coupling_bar(want_count)[..., None]
    assert np.array_equal(count, want_count) and count.min() > 0.8 * T and np.all(np.abs(mean - want_mean) <= bar)
    print(f"dense coupling: {float(np.max(np.abs(mean - want_mean) / bar)):.2e} of the bar")
    form, _ = go.coupling_kernel_form(phase.cpu().numpy())
    print(f"dense coupling against the kernel's form in numpy: {float(np.max(np.abs(mean - form) / bar)):.2e} of the bar")


# ------------------------------------------------------------------------------------------------------------------ the planted walker
def test_planted_walker(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops

    X = go.planted_walker(go.planted_pose(golden_dir))
    g = ops.gait(_dev(X, cuda), go.PLANTED["fps"])   # the default thresholds and window, the recording frame
    assert g.thresholds == (go.ON, go.OFF, go.HALF) and g.fps == go.PLANTED["fps"]
    r = {k: getattr(g, k).cpu().numpy() for k in ("tip", "vel", "states", "steps", "step_metrics", "phase", "coupling", "coupling_count", "pattern",
                                                   "pattern_histogram", "state_counts")}
    go.check_planted(r)
    # and the oracle's chain on the device's velocity: everything downstream is exact
    want = go.states_of(r["vel"][..., 0])
    assert np.array_equal(r["states"], want) and np.array_equal(r["steps"], go.steps_of(want, r["tip"], g.fps)[0])
    assert _bits(r["phase"], go.phase_of(want))
    leg, frames = go.PLANTED["missing_leg"], list(go.PLANTED["missing_frames"])
    blind = sorted({f + k for f in frames for k in (-W, W)})   # the frames whose window ends on a missing tip
    assert np.isnan(r["tip"][frames, leg]).all() and np.isnan(r["vel"][blind, leg]).all()
    assert np.isfinite(np.delete(r["vel"], leg, axis=1)).all() and np.isnan(r["vel"][:, leg, 0]).sum() == len(blind) == 4


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_determinism_guard_words_and_a_side_stream(native_lib, cuda):
    """The raw entries on sentinel-filled buffers inside guard words, the workspace too, on a stream of their own: two runs are
    bit-equal, every output element is written and nothing outside is."""
    lib = native_lib
    T = 2049 + 256   # three coupling slices, ten blocks per leg
    X, F = go.random_poses(T, seed=21), go.random_frames(T, seed=21)
    # a walker's rhythm on every tip, so that there are steps, phases and pairs to couple
    X[:, go.TIPS, 0] += 0.5 * np.sin(np.arange(T)[:, None] * (2 * np.pi / np.array([17.0, 19.0, 23.0, 17.0, 29.0, 31.0])))
    GUARD = 64
    need = lib.df3d_gait_work_bytes(T)
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

    runs = []
    with torch.cuda.stream(side):
        Xd, Fd = _dev(X, cuda), _dev(F, cuda)
        for _ in range(2):
            tip, vel, states = guarded(T * 18), guarded(T * 18), guarded(T * 6, torch.int32)
            steps, metrics, count = guarded(3 * T * 4, torch.int64), guarded(3 * T * 3), guarded(1, torch.int32)
            phase, mean, pairs = guarded(T * 6), guarded(72), guarded(36, torch.int64)
            pattern, hist, counts = guarded(T, torch.int32), guarded(64, torch.int64), guarded(18, torch.int64)
            work = guarded(need // 8)
            for rc in (lib.df3d_gait_velocity(Xd.data_ptr(), T, Fd.data_ptr(), T, FPS, W, tip[1], vel[1], st),
                       lib.df3d_gait_states(vel[1], T, 2.0, -2.0, states[1], work[1], need, st),
                       lib.df3d_gait_steps(states[1], tip[1], T, FPS, steps[1], metrics[1], count[1], work[1], need, st),
                       lib.df3d_gait_phase(states[1], T, phase[1], work[1], need, st),
                       lib.df3d_gait_coupling(phase[1], T, mean[1], pairs[1], work[1], need, st),
                       lib.df3d_gait_patterns(states[1], T, pattern[1], hist[1], counts[1], st)):
                assert rc == 0, lib.df3d_last_error()
            side.synchronize()
            inner(work[0])
            runs.append({k: inner(v[0]).copy() for k, v in dict(tip=tip, vel=vel, states=states, steps=steps, metrics=metrics, count=count,
                                                                phase=phase, mean=mean, pairs=pairs, pattern=pattern, hist=hist,
                                                                counts=counts).items()})
    first, second = runs
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), f"{k} differs between two runs"
        assert not np.any(first[k] == fills[torch.from_numpy(first[k]).dtype]), f"{k} was not written everywhere"
    want_tip, want_vel = go.tip_kinematics(X, FPS, F, W)
    vel = first["vel"].reshape(T, 6, 3)
    ok = np.isfinite(want_vel)
    assert _same_nan(vel, want_vel) and np.all(np.abs(vel - want_vel)[ok] <= go.velocity_bar(X, FPS, F, W)[ok])
    want = go.states_of(vel[..., 0], 2.0, -2.0)
    assert np.array_equal(first["states"].reshape(T, 6), want)
    S = int(first["count"][0])
    want_steps, want_metrics = go.steps_of(want, first["tip"].reshape(T, 6, 3), FPS)
    assert S == len(want_steps) > 100
    assert np.array_equal(first["steps"].reshape(3 * T, 4)[:S], want_steps) and not first["steps"].reshape(3 * T, 4)[S:].any()
    assert _bits_where_finite(first["metrics"].reshape(3 * T, 3)[:S, 2], want_metrics[:, 2]) and not first["metrics"].reshape(3 * T, 3)[S:].any()
    assert _bits(first["phase"].reshape(T, 6), go.phase_of(want))
    for k, w in zip(("pattern", "hist", "counts"), go.patterns(want)):
        assert np.array_equal(first[k].reshape(w.shape), w)
    want_mean, want_count = go.coupling(first["phase"].reshape(T, 6))
    assert np.array_equal(first["pairs"].reshape(6, 6), want_count) and want_count.min() > 0
    assert np.all(np.abs(first["mean"].reshape(6, 6, 2) - want_mean) <= go.coupling_bar(want_count)[..., None])


# ------------------------------------------------------------------------------------------------------------------ ops
def test_gait_on_non_contiguous_and_empty_input(native_lib, cuda):
    from deepfly3d_amd import ops

    T = 300
    X = go.random_poses(T, seed=5)
    X[:, go.TIPS, 0] += np.sin(np.arange(T)[:, None] * (2 * np.pi / 20.0))
    plain = ops.gait(_dev(X, cuda), FPS, on=1.0, off=-1.0)
    wide = _dev(np.repeat(X, 2, axis=2), cuda)[:, :, ::2]   # not contiguous: ops copies
    assert not wide.is_contiguous()
    again = ops.gait(wide, FPS, on=1.0, off=-1.0)
    for name in ("tip", "vel", "states", "steps", "step_metrics", "phase", "coupling", "coupling_count", "pattern", "pattern_histogram",
                 "state_counts"):
        a, b = getattr(plain, name).cpu().numpy(), getattr(again, name).cpu().numpy()
        assert _bits(a, b), name
    assert plain.steps.shape[0] > 10 and plain.thresholds == (1.0, -1.0, go.HALF) and plain.fps == FPS
    # the parts on non-contiguous views of their inputs
    vel2 = torch.stack((plain.vel, plain.vel), dim=1)[:, 0]
    states2 = torch.stack((plain.states, plain.states), dim=2)[:, :, 1]
    assert not vel2.is_contiguous() and not states2.is_contiguous()
    assert torch.equal(ops.gait_states(vel2, 1.0, -1.0), plain.states)
    assert _bits(ops.gait_phase(states2).cpu().numpy(), plain.phase.cpu().numpy())
    assert torch.equal(ops.gait_patterns(states2)[0], plain.pattern)
    empty = ops.gait(torch.zeros((0, 38, 3), dtype=torch.float64, device=cuda), FPS)
    assert empty.tip.shape == (0, 6, 3) and empty.vel.shape == (0, 6, 3) and empty.states.shape == (0, 6) and empty.states.dtype == torch.int32
    assert empty.steps.shape == (0, 4) and empty.step_metrics.shape == (0, 3) and empty.phase.shape == (0, 6) and empty.pattern.shape == (0,)
    assert torch.isnan(empty.coupling).all() and not empty.coupling_count.any() and not empty.pattern_histogram.any()
    assert not empty.state_counts.any() and empty.coupling.shape == (6, 6, 2) and empty.state_counts.shape == (6, 3)
    with pytest.raises(ValueError, match="tip must hold the 300 frames"):
        ops.gait_steps(plain.states, plain.tip[:10], FPS)
    with pytest.raises(ValueError, match=r"an explicit body_frame must be \[3, 3\] or \[T, 3, 3\]"):
        ops.tip_kinematics(_dev(X, cuda), FPS, np.zeros((5, 3, 3)))
    with pytest.raises(ValueError, match='body_frame must be "recording"'):
        ops.tip_kinematics(_dev(X, cuda), FPS, "median")


# ------------------------------------------------------------------------------------------------------------------ Core, command line
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


def _load(pkl):
    with open(pkl, "rb") as f:
        return pickle.load(f)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_keys(run, tag, thresholds, T=15):
    """The thirteen keys of one pose: shapes and types, and everything after the velocity by the host rule on the stored floats."""
    k = {name[len("gait_"):]: run[name + tag] for name in GAIT_KEYS}
    on, off, w = thresholds
    assert k["thresholds"].dtype == np.float64 and k["thresholds"].tolist() == [on, off, w] and isinstance(k["fps"], float)
    assert k["tip_position"].shape == (T, 6, 3) and k["tip_velocity"].shape == (T, 6, 3) and k["tip_velocity"].dtype == np.float64
    assert k["states"].dtype == np.int8 and k["states"].shape == (T, 6)
    want = go.states_of(k["tip_velocity"][..., 0], on, off)
    assert np.array_equal(k["states"], want)   # the host rule on the stored velocity
    steps, metrics = go.steps_of(want, k["tip_position"], k["fps"])
    assert k["steps"].dtype == np.int64 and np.array_equal(k["steps"], steps) and k["step_metrics"].shape == (len(steps), 3)
    assert _bits_where_finite(k["step_metrics"][:, 2], metrics[:, 2]) and np.all(np.abs(k["step_metrics"][:, :2] - metrics[:, :2]) <= go.duration_bar(metrics[:, :2]))
    assert _bits(k["phase"], go.phase_of(want))
    for name, w_ in zip(("pattern", "pattern_histogram", "state_counts"), go.patterns(want)):
        assert _bits(k[name], w_)
    mean, count = go.coupling(k["phase"])
    assert k["coupling_count"].dtype == np.int64 and np.array_equal(k["coupling_count"], count) and _same_nan(k["coupling"], mean)
    ok = np.isfinite(mean)
    assert np.all(np.abs(k["coupling"] - mean)[ok] <= (go.coupling_bar(count)[..., None] * np.ones(2))[ok])
    return k


def test_core_gait(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    g = core.gait(on=0.5, off=-0.5)
    assert isinstance(g, ops.GaitResult) and g.thresholds == (0.5, -0.5, cfg.GAIT_DIFF_HALF) and g.fps == cfg.SPECTROGRAM_FPS   # no videos to read a rate from
    arrays = (g.tip, g.vel, g.states, g.steps, g.step_metrics, g.phase, g.coupling, g.coupling_count, g.pattern, g.pattern_histogram, g.state_counts)
    assert all(isinstance(a, np.ndarray) for a in arrays)
    run = dict(zip(GAIT_KEYS, (g.tip, g.vel, g.states.astype(np.int8), g.steps, g.step_metrics, g.phase, g.coupling, g.coupling_count, g.pattern,
                               g.pattern_histogram, g.state_counts, np.array(g.thresholds, dtype=np.float64), g.fps)))
    _check_keys(run, "", g.thresholds)
    # the velocity against the oracle in the device's own recording frame
    X = np.ascontiguousarray(core.camNet.points3d, dtype=np.float64)
    F = ops.recording_frame(_dev(X, cuda)).cpu().numpy()[0]
    want_tip, want_vel = go.tip_kinematics(X, g.fps, F)
    ok = np.isfinite(want_vel)
    assert _same_nan(g.vel, want_vel) and _same_nan(g.tip, want_tip) and np.all(np.abs(g.vel - want_vel)[ok] <= go.velocity_bar(X, g.fps, F)[ok])
    half = core.gait(fps=50.0, half_window=1)
    assert half.fps == 50.0 and half.thresholds == (cfg.GAIT_SWING_ON, cfg.GAIT_SWING_OFF, 1)
    assert _same_nan(half.vel, go.tip_kinematics(X, 50.0, F, 1)[1])
    rigid = core.gait(rigid=True, on=0.5, off=-0.5)
    fitted = core.rigid_legs()[0]
    want_tip, want_vel = go.tip_kinematics(fitted, g.fps, F)   # the measured pose's recording frame
    ok = np.isfinite(want_vel)
    assert _same_nan(rigid.vel, want_vel) and np.all(np.abs(rigid.vel - want_vel)[ok] <= go.velocity_bar(fitted, g.fps, F)[ok])
    with pytest.raises(ValueError, match="need gait=True"):
        core.save(gait_off=-1.0)
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_gait(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd import config as cfg
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
        return _load(pkl)

    defaults = (cfg.GAIT_SWING_ON, cfg.GAIT_SWING_OFF, cfg.GAIT_DIFF_HALF)
    for others in (("--joint-angles",), ("--joint-angles", "--rigid-legs")):
        before = reopen(*others)
        run = reopen(*others, "--gait")
        tags = ("", "_rigid") if "--rigid-legs" in others else ("",)
        assert list(run.keys()) == list(before.keys()) + [k + tag for tag in tags for k in GAIT_KEYS]   # after every earlier key
        assert all(_same(before[k], run[k]) for k in before)   # every earlier key byte for byte
        for tag in tags:
            _check_keys(run, tag, defaults)
    assert not _same(run["gait_tip_velocity"], run["gait_tip_velocity_rigid"])
    alone = reopen("--gait", "--gait-on", "0.5", "--gait-off=-0.5")
    base = reopen("--joint-angles")
    assert list(alone.keys()) == [k for k in base if k not in ("joint_angles", "segment_lengths")] + GAIT_KEYS
    k = _check_keys(alone, "", (0.5, -0.5, cfg.GAIT_DIFF_HALF))
    assert _same(alone["gait_tip_velocity"], run["gait_tip_velocity"]) and k["fps"] == cfg.SPECTROGRAM_FPS
    with open(pkl, "wb") as f:
        f.write(earlier)
    with pytest.raises(SystemExit):
        cli.main([folder, "--skip-pose-estimation", "--gait-on", "3", "--order"] + order)
    with open(pkl, "rb") as f:
        assert f.read() == earlier   # refused before any work: the earlier result is untouched
    config.pop("image_shape", None)
