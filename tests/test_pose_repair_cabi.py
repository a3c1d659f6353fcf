"""CPU tests of the C entries of the pose repair (include/df3d_hip.h, a16): every refusal comes before the device is touched and names
the argument, so these run without a GPU."""
import ctypes

import pytest

A = 1 << 24   # an address that is never dereferenced: 64-byte aligned, far from the others below
STEP = 1 << 24
T = 100
T_MAX = (2 ** 31 - 1) // 38
INF, NAN = float("inf"), float("nan")


def _buffers(count):
    return [A + k * STEP for k in range(count)]


def _refused(lib, rc, fragment):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message, (rc, message)


def test_work_bytes(native_lib):
    lib = native_lib
    assert lib.df3d_repair_work_bytes(-1) == 0 and lib.df3d_repair_work_bytes(T_MAX + 1) == 0
    assert lib.df3d_repair_work_bytes(T_MAX) > 0
    sizes = [lib.df3d_repair_work_bytes(n) for n in (0, 1, 255, 256, 257, 2049, 65537, 100000)]
    assert sizes[0] >= 64 and sizes == sorted(sizes) and all(b % 64 == 0 for b in sizes)
    # the two scanned series of every joint, [76, T] int32, and their block results
    for n in (1, 257, 65537, 100000):
        blocks = (n + 255) // 256
        need = 4 * 76 * (n + blocks)
        assert need <= lib.df3d_repair_work_bytes(n) <= need + 128


def test_outliers_refusals(native_lib):
    lib = native_lib
    pts, flags, score = _buffers(3)

    def call(**kw):
        a = dict(pts=pts, T=T, h=5, scale=6.0 * 1.4826, floor=0.05, n_min=3, flags=flags, score=score)
        a.update(kw)
        return lib.df3d_repair_outliers(a["pts"], a["T"], a["h"], a["scale"], a["floor"], a["n_min"], a["flags"], a["score"], None)

    _refused(lib, call(T=-1), "T must be in [0, (2^31 - 1) / 38]")
    _refused(lib, call(T=T_MAX + 1), "T must be in")
    for h in (0, -1, 65):
        _refused(lib, call(h=h), "half_window must be in [1, 64]")
    for scale in (0.0, -1.0, INF, NAN):
        _refused(lib, call(scale=scale), "scale must be finite and > 0")
    for floor in (-0.01, INF, -INF, NAN):
        _refused(lib, call(floor=floor), "floor must be finite and >= 0")
    for h, n_min in ((5, 0), (5, 12), (1, 4), (64, 130), (5, -3)):
        _refused(lib, call(h=h, n_min=n_min), "min_count must be in [1, 2 half_window + 1]")
    for name in ("pts", "flags"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(pts=pts + 4), "pts must be 8-byte aligned")
    _refused(lib, call(score=score + 4), "score must be 8-byte aligned")
    _refused(lib, call(flags=pts + T * 38 * 24 - 1), "flags must not overlap pts")
    _refused(lib, call(score=pts + 8), "score must not overlap pts")
    _refused(lib, call(score=flags + T * 38 - 6), "score must be 8-byte aligned")
    _refused(lib, call(score=flags + T * 38 - 8), "score must not overlap flags")
    # no frames: nothing to do, whatever the pointers; the parameters are still checked
    assert lib.df3d_repair_outliers(None, 0, 5, 8.0, 0.05, 3, None, None, None) == 0
    _refused(lib, lib.df3d_repair_outliers(None, 0, 5, 8.0, -1.0, 3, None, None, None), "floor must be finite")
    # a null score is allowed: with the other arguments valid the call goes on to the device, so only its checks are exercised here
    _refused(lib, call(score=None, flags=None), "null pointer: flags")


def test_fill_refusals(native_lib):
    lib = native_lib
    pts, flags, out, status, counts, work = _buffers(6)
    need = lib.df3d_repair_work_bytes(T)

    def call(**kw):
        a = dict(pts=pts, flags=flags, T=T, gap=10, out=out, status=status, counts=counts, work=work, need=need)
        a.update(kw)
        return lib.df3d_repair_fill(a["pts"], a["flags"], a["T"], a["gap"], a["out"], a["status"], a["counts"], a["work"], a["need"], None)

    _refused(lib, call(T=-1), "T must be in [0, (2^31 - 1) / 38]")
    _refused(lib, call(T=T_MAX + 1), "T must be in")
    for gap in (-1, 1000001):
        _refused(lib, call(gap=gap), "max_gap must be in [0, 1000000]")
    _refused(lib, call(need=need - 1), "work buffer too small (df3d_repair_work_bytes)")
    _refused(lib, call(need=0), "work buffer too small (df3d_repair_work_bytes)")
    for name in ("pts", "flags", "out", "status", "counts", "work"):
        _refused(lib, call(**{name: None}), f"null pointer: {name}")
    _refused(lib, call(pts=pts + 4), "pts must be 8-byte aligned")
    _refused(lib, call(out=out + 4), "out must be 8-byte aligned")
    _refused(lib, call(counts=counts + 4), "counts must be 8-byte aligned")
    _refused(lib, call(work=work + 8), "work must be 16-byte aligned")
    _refused(lib, call(out=pts), "out must not overlap pts")   # never in place: a filled value reads its neighbours
    _refused(lib, call(out=pts + T * 38 * 24 - 8), "out must not overlap pts")
    _refused(lib, call(status=flags + T * 38 - 1), "status must not overlap flags")
    _refused(lib, call(counts=out + 8), "counts must not overlap out")
    _refused(lib, call(work=counts + 38 * 5 * 8 - 16), "work must not overlap counts")
    _refused(lib, call(work=status - need + 16), "work must not overlap status")
    assert lib.df3d_repair_fill(None, None, 0, 10, None, None, None, None, 0, None) == 0
    _refused(lib, lib.df3d_repair_fill(None, None, 0, -1, None, None, None, None, 0, None), "max_gap must be in")


def test_the_entries_are_exported_with_their_prototypes(native_lib):
    from deepfly3d_amd import _native

    for name in ("df3d_repair_work_bytes", "df3d_repair_outliers", "df3d_repair_fill"):
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == 610
    with pytest.raises(ctypes.ArgumentError):
        native_lib.df3d_repair_work_bytes("many")
