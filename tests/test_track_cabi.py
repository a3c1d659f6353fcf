"""CPU tests of the two C entries of the tracking solve (include/df3d_hip.h, a18): every refusal comes before the device is touched and
names the argument, so these run without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 28   # addresses that are never dereferenced: 64-byte aligned, far from one another
STEP = 1 << 28
C, T, J, K = 7, 100, 19, 10
INF, NAN = float("inf"), float("nan")
NAMES = ("df3d_track_work_bytes", "df3d_track_peaks")


def _refused(lib, rc, fragment):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message and message.startswith("df3d_track_peaks: "), (rc, message)


def _call(lib, **kw):
    count, pts, val, choice, cost, work = (A + n * STEP for n in range(6))
    a = dict(count=count, pts=pts, val=val, C=C, T=T, J=J, K=K, H=480.0, W=960.0, tau=30.0, wm=1.0, wv=1.0, block=256, choice=choice, cost=cost,
             work=work)
    a.update(kw)
    if "need" not in a:
        a["need"] = max(lib.df3d_track_work_bytes(a["C"] * a["J"], a["T"], a["K"], a["block"]), 0)
    return lib.df3d_track_peaks(a["count"], a["pts"], a["val"], a["C"], a["T"], a["J"], a["K"], a["H"], a["W"], a["tau"], a["wm"], a["wv"], a["block"],
                                a["choice"], a["cost"], a["work"], a["need"], None)


def test_work_bytes(native_lib):
    lib = native_lib
    n = C * J
    for bad in ((0, T, K, 256), (-1, T, K, 256), ((1 << 20) + 1, 1, K, 256), (n, -1, K, 256), (n, 1 << 31, K, 256), (1 << 20, (1 << 16) + 1, K, 256),
                (n, T, 0, 256), (n, T, 17, 256), (n, T, K, 0), (n, T, K, 4097)):
        assert lib.df3d_track_work_bytes(*bad) == 0, bad
    assert lib.df3d_track_work_bytes(1 << 20, 1 << 16, 16, 4096) > 0 and lib.df3d_track_work_bytes(1, (1 << 31) - 1, 1, 1) > 0
    for frames, block in ((1, 1), (1, 256), (255, 256), (256, 256), (257, 256), (300, 64), (20000, 256), (100000, 4096)):
        blocks = -(-frames // block)
        need = lib.df3d_track_work_bytes(n, frames, K, block)
        # per (chain, block): a [16, 16] int64 transfer matrix, a [16] int64 vector, 16 map bytes and the exit state; per (chain, frame):
        # 16 back-pointers; per chain: the last state.  Six parts, each rounded up to 64 bytes
        exact = n * blocks * (2048 + 128 + 16 + 1) + n * frames * 16 + n * 4
        assert need % 64 == 0 and exact <= need < exact + 6 * 64, (frames, block)
    assert lib.df3d_track_work_bytes(n, 0, K, 256) >= 0
    assert lib.df3d_track_work_bytes(n, T, 1, 256) == lib.df3d_track_work_bytes(n, T, 16, 256)   # K is padded to 16 states


def test_refusals(native_lib):
    lib = native_lib
    for name in ("C", "J"):
        for v in (0, -1):
            _refused(lib, _call(lib, **{name: v}), "C and J must be >= 1")
    _refused(lib, _call(lib, C=1 << 11, J=1 << 10), "C J at most 2^20")
    _refused(lib, _call(lib, T=-1), "T must be in [0, 2^31 - 1]")
    _refused(lib, _call(lib, T=1 << 31), "T must be in [0, 2^31 - 1]")
    _refused(lib, _call(lib, C=1 << 10, J=1 << 10, T=(1 << 16) + 1), "C J T at most 2^36")
    for k in (0, 17, -1):
        _refused(lib, _call(lib, K=k), "K must be in [1, 16]")
    for name in ("H", "W"):
        for v in (0.0, -480.0, INF, NAN):
            _refused(lib, _call(lib, **{name: v}), "height_px and width_px must be finite and > 0")
    for tau in (0.0, -30.0, NAN, INF):
        _refused(lib, _call(lib, tau=tau), "tau must be finite and > 0")
    for w in (-1e-9, 1024.5, NAN, INF, -INF):
        _refused(lib, _call(lib, wm=w), "w_motion must be finite and in [0, 1024]")
        _refused(lib, _call(lib, wv=w), "w_value must be finite and in [0, 1024]")
    for block in (0, 4097, -256):
        _refused(lib, _call(lib, block=block, need=1 << 40), "block_frames must be in [1, 4096]")
    # the overflow bound: T (w_m + w_v) 2^20 < 2^60.  2^29 frames at the largest weights reach it, one frame fewer does not
    _refused(lib, _call(lib, C=1, J=1, T=1 << 29, wm=1024.0, wv=1024.0, block=4096), "T (w_motion + w_value) 2^20 must be below 2^60")
    _refused(lib, _call(lib, C=1, J=1, T=(1 << 29) - 1, wm=1024.0, wv=1024.0, block=4096, count=None), "null pointer: count")
    _refused(lib, _call(lib, C=1, J=1, T=1 << 30, wm=512.0, wv=512.0, block=4096), "T (w_motion + w_value) 2^20 must be below 2^60")
    _refused(lib, _call(lib, C=1 << 10, J=1, T=1 << 22, block=1, need=1 << 60), "use larger blocks")
    need = lib.df3d_track_work_bytes(C * J, T, K, 256)
    _refused(lib, _call(lib, need=need - 1), "work buffer too small (df3d_track_work_bytes)")
    _refused(lib, _call(lib, need=0), "work buffer too small (df3d_track_work_bytes)")
    for name in ("count", "pts", "val", "choice", "cost", "work"):
        _refused(lib, _call(lib, **{name: None}), f"null pointer: {name}")
    _refused(lib, _call(lib, count=A + 2), "count must be 4-byte aligned")
    _refused(lib, _call(lib, pts=A + STEP + 1), "pts must be 4-byte aligned")
    _refused(lib, _call(lib, cost=A + 4 * STEP + 4), "cost must be 8-byte aligned")
    _refused(lib, _call(lib, work=A + 5 * STEP + 8), "work must be 16-byte aligned")
    _refused(lib, _call(lib, choice=A + C * T * J * 4 - 4), "choice must not overlap count")
    _refused(lib, _call(lib, val=A + STEP + C * T * J * K * 8 - 4), "val must not overlap pts")
    _refused(lib, _call(lib, cost=A + 3 * STEP + C * T * J * 4 - 8), "cost must not overlap choice")
    _refused(lib, _call(lib, work=A + 4 * STEP + C * J * 8 - 8), "work must not overlap cost")
    _refused(lib, _call(lib, work=A + 2 * STEP - need + 16), "work must not overlap val")


def test_no_frames_succeed(native_lib):
    lib = native_lib
    assert lib.df3d_track_peaks(None, None, None, C, 0, J, K, 480.0, 960.0, 30.0, 1.0, 1.0, 256, None, None, None, 0, None) == 0
    # ... but the parameters are still checked
    _refused(lib, lib.df3d_track_peaks(None, None, None, C, 0, J, 17, 480.0, 960.0, 30.0, 1.0, 1.0, 256, None, None, None, 0, None), "K must be in")
    _refused(lib, lib.df3d_track_peaks(None, None, None, C, 0, J, K, 480.0, 960.0, 0.0, 1.0, 1.0, 256, None, None, None, 0, None), "tau must be")


def test_the_entries_are_exported_and_the_abi_stays(native_lib):
    from deepfly3d_amd import _native

    for name in NAMES:
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == _native.ABI_VERSION == 610
    assert _native.PROTOTYPES["df3d_track_work_bytes"] == (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int])
    text = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    assert re.search(r"#define\s+DF3D_ABI_VERSION\s+610\b", text) and "a18 tracking of the 2-D detections" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        declared = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code)
        assert declared and len(declared.group(1).split(",")) == len(_native.PROTOTYPES[name][1]), name
