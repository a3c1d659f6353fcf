"""CPU tests of the C entries of the treadmill analysis (include/df3d_hip.h, a17): every refusal comes before the device is touched
and names the argument, so these run without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 24   # an address that is never dereferenced: 64-byte aligned, far from the others below
STEP = 1 << 24
T = 100
T_MAX = (2 ** 31 - 1) // 6
INF, NAN = float("inf"), float("nan")
NAMES = ("df3d_ball_work_bytes", "df3d_ball_tips", "df3d_ball_fit", "df3d_ball_rotation", "df3d_ball_path")


def _buffers(count):
    return [A + k * STEP for k in range(count)]


def _refused(lib, rc, fragment):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message, (rc, message)


def test_work_bytes(native_lib):
    lib = native_lib
    assert lib.df3d_ball_work_bytes(-1) == 0 and lib.df3d_ball_work_bytes(T_MAX + 1) == 0 and lib.df3d_ball_work_bytes(T_MAX) > 0
    sizes = [lib.df3d_ball_work_bytes(n) for n in (0, 1, 255, 256, 257, 341, 342, 2048, 2049, 65537, 100000)]
    assert sizes[0] >= 64 and sizes == sorted(sizes) and all(b % 64 == 0 for b in sizes)
    for n in (1, 342, 65537, 100000):
        slices, blocks = (6 * n + 2047) // 2048, (n + 255) // 256
        # a [16] partial per slice of 2 048 samples, the parameter block, and the block results of a two-row scan
        assert lib.df3d_ball_work_bytes(n) >= 8 * (16 * slices + 64 + 2 * blocks)
    # the slice is a constant of the file: 342 frames are 2 052 samples, one more slice than 341
    assert lib.df3d_ball_work_bytes(342) - lib.df3d_ball_work_bytes(341) == 16 * 8


def test_tips_refusals(native_lib):
    lib = native_lib
    pts, frame, coxa, tip, vel = _buffers(5)

    def call(**kw):
        a = dict(pts=pts, T=T, frame=frame, coxa=coxa, fps=100.0, w=2, tip=tip, vel=vel)
        a.update(kw)
        return lib.df3d_ball_tips(a["pts"], a["T"], a["frame"], a["coxa"], a["fps"], a["w"], a["tip"], a["vel"], None)

    _refused(lib, call(T=-1), "T must be in")
    _refused(lib, call(T=T_MAX + 1), "T must be in")
    for fps in (0.0, -100.0, INF, NAN):
        _refused(lib, call(fps=fps), "fps must be finite and > 0")
    for w in (0, -1, 65):
        _refused(lib, call(w=w), "half_window must be in [1, 64]")
    for name in ("pts", "frame", "coxa", "tip", "vel"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
        _refused(lib, call(**{name: A + 4 + 7 * STEP}), f"{name} must be 8-byte aligned")
    _refused(lib, call(tip=pts + T * 38 * 24 - 8), "tip must not overlap pts")
    _refused(lib, call(vel=tip + 8), "vel must not overlap tip")
    _refused(lib, call(vel=frame + 64), "vel must not overlap frame")
    _refused(lib, call(coxa=frame + 64), "coxa must not overlap frame")
    _refused(lib, call(tip=coxa + 6 * 24 - 8), "tip must not overlap coxa")
    assert lib.df3d_ball_tips(None, 0, None, None, 100.0, 2, None, None, None) == 0   # no frames: nothing to do, whatever the pointers
    _refused(lib, lib.df3d_ball_tips(None, 0, None, None, 0.0, 2, None, None, None), "fps must be finite")


def test_fit_refusals(native_lib):
    lib = native_lib
    tip, states, ball, info, sums, work = _buffers(6)
    need = lib.df3d_ball_work_bytes(T)

    def call(**kw):
        a = dict(tip=tip, states=states, T=T, known=1, radius=5.0, iterations=8, pivot=1e-10, ball=ball, info=info, sums=sums, work=work, need=need)
        a.update(kw)
        return lib.df3d_ball_fit(a["tip"], a["states"], a["T"], a["known"], a["radius"], a["iterations"], a["pivot"], a["ball"], a["info"], a["sums"],
                                 a["work"], a["need"], None)

    _refused(lib, call(T=-1), "T must be in")
    _refused(lib, call(T=T_MAX + 1), "T must be in")
    for known in (-1, 2):
        _refused(lib, call(known=known), "known_radius must be 0 or 1")
    for radius in (0.0, -5.0, INF, NAN):
        _refused(lib, call(radius=radius), "radius must be finite and > 0")
    for iterations in (0, -1, 65):
        _refused(lib, call(iterations=iterations), "iterations must be in [1, 64]")
    for pivot in (-1e-10, 1.0, NAN, INF):
        _refused(lib, call(pivot=pivot), "pivot_min must be in [0, 1)")
    _refused(lib, call(need=need - 1), "work buffer too small (df3d_ball_work_bytes)")
    for name in ("tip", "states", "ball", "info", "sums", "work"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(tip=tip + 4), "tip must be 8-byte aligned")
    _refused(lib, call(states=states + 2), "states must be 4-byte aligned")
    _refused(lib, call(info=info + 4), "info must be 8-byte aligned")
    _refused(lib, call(work=work + 8), "work must be 16-byte aligned")
    _refused(lib, call(states=tip + T * 6 * 24 - 4), "states must not overlap tip")
    _refused(lib, call(info=ball + 56), "info must not overlap ball")
    _refused(lib, call(sums=info + 8), "sums must not overlap info")
    _refused(lib, call(work=sums + 17 * 8 - 8), "work must not overlap sums")
    _refused(lib, call(work=states - need + 16), "work must not overlap states")
    # a free radius looks at neither the radius nor the iterations, and passes every check down to the first buffer
    _refused(lib, call(known=0, radius=NAN, iterations=0, tip=None), "null pointer: tip")
    assert lib.df3d_ball_fit(None, None, 0, 0, 0.0, 0, 1e-10, None, None, None, None, 0, None) == 0
    _refused(lib, lib.df3d_ball_fit(None, None, 0, 1, -1.0, 8, 1e-10, None, None, None, None, 0, None), "radius must be finite")


def test_rotation_refusals(native_lib):
    lib = native_lib
    tip, vel, states, ball, omega, legs, residual, fictive = _buffers(8)

    def call(**kw):
        a = dict(tip=tip, vel=vel, states=states, T=T, ball=ball, min_legs=2, pivot=1e-10, omega=omega, legs=legs, residual=residual, fictive=fictive)
        a.update(kw)
        return lib.df3d_ball_rotation(a["tip"], a["vel"], a["states"], a["T"], a["ball"], a["min_legs"], a["pivot"], a["omega"], a["legs"],
                                      a["residual"], a["fictive"], None)

    _refused(lib, call(T=-1), "T must be in")
    for min_legs in (1, 0, 7, -2):
        _refused(lib, call(min_legs=min_legs), "min_legs must be in [2, 6]")
    for pivot in (-1.0, 1.0, NAN):
        _refused(lib, call(pivot=pivot), "pivot_min must be in [0, 1)")
    for name in ("tip", "vel", "states", "ball", "omega", "legs", "residual", "fictive"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(omega=omega + 4), "omega must be 8-byte aligned")
    _refused(lib, call(legs=legs + 2), "legs must be 4-byte aligned")
    _refused(lib, call(omega=tip + T * 6 * 24 - 8), "omega must not overlap tip")
    _refused(lib, call(omega=ball + 56), "omega must not overlap ball")
    _refused(lib, call(legs=omega + T * 24 - 4), "legs must not overlap omega")
    _refused(lib, call(fictive=residual + T * 8 - 8), "fictive must not overlap residual")
    _refused(lib, call(residual=vel + 8), "residual must not overlap vel")
    assert lib.df3d_ball_rotation(None, None, None, 0, None, 2, 1e-10, None, None, None, None, None) == 0
    _refused(lib, lib.df3d_ball_rotation(None, None, None, 0, None, 1, 1e-10, None, None, None, None, None), "min_legs must be in")


def test_path_refusals(native_lib):
    lib = native_lib
    fictive, path, skipped, work = _buffers(4)
    need = lib.df3d_ball_work_bytes(T)

    def call(**kw):
        a = dict(fictive=fictive, T=T, fps=100.0, path=path, skipped=skipped, work=work, need=need)
        a.update(kw)
        return lib.df3d_ball_path(a["fictive"], a["T"], a["fps"], a["path"], a["skipped"], a["work"], a["need"], None)

    _refused(lib, call(T=-1), "T must be in")
    for fps in (0.0, NAN, -INF):
        _refused(lib, call(fps=fps), "fps must be finite and > 0")
    _refused(lib, call(need=need - 64), "work buffer too small (df3d_ball_work_bytes)")
    for name in ("fictive", "path", "skipped", "work"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(path=path + 4), "path must be 8-byte aligned")
    _refused(lib, call(skipped=skipped + 4), "skipped must be 8-byte aligned")
    _refused(lib, call(work=work + 8), "work must be 16-byte aligned")
    _refused(lib, call(path=fictive + T * 24 - 8), "path must not overlap fictive")
    _refused(lib, call(skipped=path + 16), "skipped must not overlap path")
    _refused(lib, call(work=skipped - need + 16), "work must not overlap skipped")
    assert lib.df3d_ball_path(None, 0, 100.0, None, None, None, 0, None) == 0


def test_the_entries_are_exported_with_their_prototypes(native_lib):
    from deepfly3d_amd import _native

    for name in NAMES:
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == _native.ABI_VERSION == 610
    with pytest.raises(ctypes.ArgumentError):
        native_lib.df3d_ball_work_bytes("many")


def test_header_and_prototypes_agree():
    """Section a17 of the header declares the five entries, each with as many arguments as its prototype, and leaves the ABI at 610."""
    from deepfly3d_amd import _native

    text = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    assert re.search(r"#define\s+DF3D_ABI_VERSION\s+610\b", text)
    assert "a17 the treadmill ball" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        declared = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code)
        assert declared, name
        assert len(declared.group(1).split(",")) == len(_native.PROTOTYPES[name][1]), name
    assert _native.PROTOTYPES["df3d_ball_work_bytes"] == (ctypes.c_longlong, [ctypes.c_longlong])
