"""CPU tests of the C entries of the gait analysis (include/df3d_hip.h, a15): every refusal comes before the device is touched and
names the argument, so these run without a GPU."""
import ctypes

import pytest

A = 1 << 24   # an address that is never dereferenced: 64-byte aligned, far from the others below
STEP = 1 << 24
T = 100
INF, NAN = float("inf"), float("nan")


def _buffers(count):
    return [A + k * STEP for k in range(count)]


def _refused(lib, rc, fragment):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message, (rc, message)


def test_work_bytes(native_lib):
    lib = native_lib
    assert lib.df3d_gait_work_bytes(-1) == 0 and lib.df3d_gait_work_bytes((2 ** 31 - 1) // 6 + 1) == 0
    assert lib.df3d_gait_work_bytes((2 ** 31 - 1) // 6) > 0
    sizes = [lib.df3d_gait_work_bytes(n) for n in (0, 1, 255, 256, 257, 2048, 2049, 65537, 100000)]
    assert sizes[0] >= 64 and sizes == sorted(sizes) and all(b % 64 == 0 for b in sizes)
    # the four scanned series and the flags with their numbers, [6, T] int32 each, and the scans' block results
    for n in (1, 257, 65537, 100000):
        blocks = (n + 255) // 256
        assert lib.df3d_gait_work_bytes(n) >= 4 * (6 * 6 * n + 24 * blocks + (6 * n + 255) // 256)
    # the coupling's share grows by one [36, 3] partial per 2 048 frames: the slice is a constant of the file
    base = lib.df3d_gait_work_bytes(2048) - 64 * ((36 * 3 * 8 + 63) // 64)
    assert lib.df3d_gait_work_bytes(100000) >= base + 49 * 36 * 3 * 8


def test_velocity_refusals(native_lib):
    lib = native_lib
    pts, frame, tip, vel = _buffers(4)

    def call(**kw):
        a = dict(pts=pts, T=T, frame=frame, nframes=1, fps=100.0, w=2, tip=tip, vel=vel)
        a.update(kw)
        return lib.df3d_gait_velocity(a["pts"], a["T"], a["frame"], a["nframes"], a["fps"], a["w"], a["tip"], a["vel"], None)

    _refused(lib, call(T=-1), "T must be in")
    _refused(lib, call(T=(2 ** 31 - 1) // 6 + 1), "T must be in")
    for fps in (0.0, -100.0, INF, NAN):
        _refused(lib, call(fps=fps), "fps must be finite and > 0")
    for w in (0, -1, 65):
        _refused(lib, call(w=w), "half_window must be in [1, 64]")
    for nframes in (0, 2, T - 1, T + 1, -1):
        _refused(lib, call(nframes=nframes), "nframes must be 1")
    for name in ("pts", "frame", "tip", "vel"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
        _refused(lib, call(**{name: A + 4 + 5 * STEP}), f"{name} must be 8-byte aligned")
    _refused(lib, call(tip=pts + T * 38 * 24 - 8), "tip must not overlap pts")
    _refused(lib, call(vel=tip + 8), "vel must not overlap tip")
    _refused(lib, call(vel=frame + 64), "vel must not overlap frame")
    _refused(lib, call(nframes=T, tip=frame + T * 72 - 8), "tip must not overlap frame")
    assert lib.df3d_gait_velocity(None, 0, None, 1, 100.0, 2, None, None, None) == 0   # no frames: nothing to do, whatever the pointers
    _refused(lib, lib.df3d_gait_velocity(None, 0, None, 1, 0.0, 2, None, None, None), "fps must be finite")


def test_states_refusals(native_lib):
    lib = native_lib
    vel, states, work = _buffers(3)
    need = lib.df3d_gait_work_bytes(T)

    def call(**kw):
        a = dict(vel=vel, T=T, on=5.0, off=0.0, states=states, work=work, need=need)
        a.update(kw)
        return lib.df3d_gait_states(a["vel"], a["T"], a["on"], a["off"], a["states"], a["work"], a["need"], None)

    _refused(lib, call(T=-3), "T must be in")
    for on, off in ((NAN, 0.0), (5.0, NAN), (INF, 0.0), (5.0, -INF)):
        _refused(lib, call(on=on, off=off), "on and off must be finite")
    for on, off in ((0.0, 0.0), (1.0, 2.0)):
        _refused(lib, call(on=on, off=off), "on must be above off")
    _refused(lib, call(need=need - 1), "work buffer too small (df3d_gait_work_bytes)")
    for name in ("vel", "states", "work"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(vel=vel + 4), "vel must be 8-byte aligned")
    _refused(lib, call(states=states + 2), "states must be 4-byte aligned")
    _refused(lib, call(work=work + 8), "work must be 16-byte aligned")
    _refused(lib, call(states=vel + T * 6 * 24 - 4), "states must not overlap vel")
    _refused(lib, call(work=states - need + 16), "work must not overlap states")
    assert lib.df3d_gait_states(None, 0, 5.0, 0.0, None, None, 0, None) == 0


def test_steps_and_phase_refusals(native_lib):
    lib = native_lib
    states, tip, steps, metrics, count, work, phase = _buffers(7)
    need = lib.df3d_gait_work_bytes(T)

    def call(**kw):
        a = dict(states=states, tip=tip, T=T, fps=100.0, steps=steps, metrics=metrics, count=count, work=work, need=need)
        a.update(kw)
        return lib.df3d_gait_steps(a["states"], a["tip"], a["T"], a["fps"], a["steps"], a["metrics"], a["count"], a["work"], a["need"], None)

    _refused(lib, call(T=-1), "T must be in")
    for fps in (0.0, NAN, -INF):
        _refused(lib, call(fps=fps), "fps must be finite and > 0")
    _refused(lib, call(need=need - 1), "work buffer too small (df3d_gait_work_bytes)")
    for name, message in (("states", "states"), ("tip", "tip"), ("steps", "steps"), ("metrics", "metrics"), ("count", "num_steps"), ("work", "work")):
        _refused(lib, call(**{name: None}), f"null pointer: {message}")
    _refused(lib, call(steps=steps + 4), "steps must be 8-byte aligned")
    _refused(lib, call(count=count + 2), "num_steps must be 4-byte aligned")
    _refused(lib, call(metrics=steps + 3 * T * 32 - 8), "metrics must not overlap steps")   # steps holds 3 T rows of four int64
    _refused(lib, call(count=metrics + 3 * T * 24 - 4), "num_steps must not overlap metrics")
    _refused(lib, call(steps=tip + 8), "steps must not overlap tip")
    assert lib.df3d_gait_steps(None, None, 0, 100.0, None, None, None, None, 0, None) == 0

    def call_phase(**kw):
        a = dict(states=states, T=T, phase=phase, work=work, need=need)
        a.update(kw)
        return lib.df3d_gait_phase(a["states"], a["T"], a["phase"], a["work"], a["need"], None)

    _refused(lib, call_phase(T=-1), "T must be in")
    _refused(lib, call_phase(need=0), "work buffer too small (df3d_gait_work_bytes)")
    for name in ("states", "phase", "work"):
        _refused(lib, call_phase(**{name: None}), f"null pointer: {name}")
    _refused(lib, call_phase(phase=phase + 4), "phase must be 8-byte aligned")
    _refused(lib, call_phase(phase=states + 16), "phase must not overlap states")
    assert lib.df3d_gait_phase(None, 0, None, None, 0, None) == 0


def test_coupling_and_patterns_refusals(native_lib):
    lib = native_lib
    phase, mean, count, work, states, pattern, hist, counts = _buffers(8)
    need = lib.df3d_gait_work_bytes(T)

    def call(**kw):
        a = dict(phase=phase, T=T, mean=mean, count=count, work=work, need=need)
        a.update(kw)
        return lib.df3d_gait_coupling(a["phase"], a["T"], a["mean"], a["count"], a["work"], a["need"], None)

    _refused(lib, call(T=-1), "T must be in")
    _refused(lib, call(need=need - 64), "work buffer too small (df3d_gait_work_bytes)")
    for name in ("phase", "mean", "count", "work"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(mean=mean + 4), "mean must be 8-byte aligned")
    _refused(lib, call(count=mean + 36 * 16 - 8), "count must not overlap mean")
    _refused(lib, call(mean=phase + T * 48 - 8), "mean must not overlap phase")
    assert lib.df3d_gait_coupling(None, 0, None, None, None, 0, None) == 0

    def call_patterns(**kw):
        a = dict(states=states, T=T, pattern=pattern, hist=hist, counts=counts)
        a.update(kw)
        return lib.df3d_gait_patterns(a["states"], a["T"], a["pattern"], a["hist"], a["counts"], None)

    _refused(lib, call_patterns(T=-1), "T must be in")
    for name, message in (("states", "states"), ("pattern", "pattern"), ("hist", "histogram"), ("counts", "state_counts")):
        _refused(lib, call_patterns(**{name: None}), f"null pointer: {message}")
    _refused(lib, call_patterns(hist=hist + 4), "histogram must be 8-byte aligned")
    _refused(lib, call_patterns(pattern=pattern + 1), "pattern must be 4-byte aligned")
    _refused(lib, call_patterns(counts=hist + 64 * 8 - 8), "state_counts must not overlap histogram")
    _refused(lib, call_patterns(pattern=states + T * 24 - 4), "pattern must not overlap states")
    assert lib.df3d_gait_patterns(None, 0, None, None, None, None) == 0


def test_the_entries_are_exported_with_their_prototypes(native_lib):
    from deepfly3d_amd import _native

    names = ("df3d_gait_work_bytes", "df3d_gait_velocity", "df3d_gait_states", "df3d_gait_steps", "df3d_gait_phase", "df3d_gait_coupling",
             "df3d_gait_patterns")
    for name in names:
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == 610
    with pytest.raises(ctypes.ArgumentError):
        native_lib.df3d_gait_work_bytes("many")
