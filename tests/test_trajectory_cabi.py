"""CPU tests of the four C entries of the trajectory triangulation (include/df3d_hip.h, a20): every refusal comes before the device is
touched and carries a message, so these run without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 28   # addresses that are never dereferenced: 64-byte aligned, far from one another
STEP = 1 << 28
NCAM, T, J, B = 7, 100, 38, 16
INF, NAN = float("inf"), float("nan")
NAMES = ("df3d_trajectory_work_bytes", "df3d_trajectory_linearize", "df3d_trajectory_solve", "df3d_triangulate_trajectory")
DP = ctypes.POINTER(ctypes.c_double)
FIT, LIN, SOLVE = NAMES[3], NAMES[1], NAMES[2]


def _refused(lib, rc, fragment, entry=FIT):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message and message.startswith(entry + ": "), (rc, message)


def _doubles(values):
    return (ctypes.c_double * len(values))(*values)


def _host(v):
    return v if v is None else ctypes.cast(v, DP)


def _fit(lib, **kw):
    names = ("pts", "X0", "X", "status", "weight", "err", "iterations", "cost", "counts", "work")
    a = dict(P=_doubles([1.0] * 96), ncam=NCAM, T=T, J=J, lam=_doubles([1e4] * 64), delta=10.0, max_gap=10, B=B)
    a.update({n: A + k * STEP for k, n in enumerate(names)})
    a.update(kw)
    if "need" not in a:
        a["need"] = max(lib.df3d_trajectory_work_bytes(NCAM, max(a["T"], 0), J, B), 0)
    return lib.df3d_triangulate_trajectory(_host(a["P"]), a["pts"], a["X0"], a["ncam"], a["T"], a["J"], _host(a["lam"]), a["delta"], a["max_gap"],
                                           a["B"], a["X"], a["status"], a["weight"], a["err"], a["iterations"], a["cost"], a["counts"], a["work"],
                                           a["need"], None)


def _linearize(lib, **kw):
    names = ("pts", "X", "H", "g", "weight", "err", "cost", "work")
    a = dict(P=_doubles([1.0] * 96), ncam=NCAM, T=T, J=J, delta=10.0, need=T * J * 8)
    a.update({n: A + k * STEP for k, n in enumerate(names)})
    a.update(kw)
    return lib.df3d_trajectory_linearize(_host(a["P"]), a["pts"], a["X"], a["ncam"], a["T"], a["J"], a["delta"], a["H"], a["g"], a["weight"], a["err"],
                                         a["cost"], a["work"], a["need"], None)


def _solve(lib, **kw):
    names = ("H", "g", "segment", "d", "ok", "work", "ticks")
    a = dict(T=T, J=J, lam=_doubles([1e4] * 64), mu=1e-3, B=B)
    a.update({n: A + k * STEP for k, n in enumerate(names)})
    a.update(kw)
    if "need" not in a:
        a["need"] = max(lib.df3d_trajectory_work_bytes(1, max(a["T"], 0), J, B), 0)
    return lib.df3d_trajectory_solve(a["H"], a["g"], a["segment"], a["T"], a["J"], _host(a["lam"]), a["mu"], a["B"], a["d"], a["ok"], a["ticks"],
                                     a["work"], a["need"], None)


def test_work_bytes(native_lib):
    lib = native_lib
    for bad in ((0, T, J, B), (9, T, J, B), (NCAM, -1, J, B), (NCAM, (1 << 20) + 1, J, B), (NCAM, T, 0, B), (NCAM, T, 65, B), (NCAM, T, J, 2),
                (NCAM, T, J, (1 << 20) + 1)):
        assert lib.df3d_trajectory_work_bytes(*bad) == 0, bad
    assert lib.df3d_trajectory_work_bytes(NCAM, 0, J, B) == 0
    for frames, block in ((1, 3), (2, 16), (100, 16), (257, 3), (1000, 64), (1000, 1 << 20)):
        bc = min(block, max(frames, 3))
        nb = -(-frames // bc)
        tj = frames * J
        exact = 8 * (13 * tj + (tj * 10 + 63) // 64 * 8 + J * (48 * nb * bc + 105 * nb))
        assert lib.df3d_trajectory_work_bytes(NCAM, frames, J, block) == exact, (frames, block)
    assert lib.df3d_trajectory_work_bytes(1, T, J, B) == lib.df3d_trajectory_work_bytes(8, T, J, B)
    assert lib.df3d_trajectory_work_bytes(NCAM, 1 << 20, 64, 3) > 1 << 34     # no 32-bit overflow at the largest shape


def test_fit_refusals(native_lib):
    lib = native_lib
    for ncam in (0, 9, -1):
        _refused(lib, _fit(lib, ncam=ncam, need=1 << 40), "ncam must be in [1, 8]")
    for j in (0, 65):
        _refused(lib, _fit(lib, J=j, need=1 << 40), "J must be in [1, 64]")
    for frames in (-1, (1 << 20) + 1):
        _refused(lib, _fit(lib, T=frames, need=1 << 40), "T must be in [0, 1048576]")
    for block in (2, 0, -1, (1 << 20) + 1):
        _refused(lib, _fit(lib, B=block), "block_frames must be in [3, 1048576]")
    for bad in (NAN, -1.0, -INF):
        _refused(lib, _fit(lib, delta=bad), "delta must be >= 0 and not NaN")
    for bad in (-1, 1000001):
        _refused(lib, _fit(lib, max_gap=bad), "max_gap must be in [0, 1000000]")
    for bad in (NAN, -1.0, INF, -INF):
        _refused(lib, _fit(lib, lam=_doubles([1e4] * 37 + [bad] + [1e4] * 26)), "lambda must be >= 0 and finite")
    assert _fit(lib, T=0, lam=_doubles([0.0, 1e12] * 32), delta=INF, max_gap=0) == 0   # 0, a large lambda and delta = +inf are values
    _refused(lib, _fit(lib, P=None), "null pointer: P_host")
    _refused(lib, _fit(lib, lam=None), "null pointer: lambda_host")
    need = lib.df3d_trajectory_work_bytes(NCAM, T, J, B)
    _refused(lib, _fit(lib, need=need - 1), "work buffer too small (df3d_trajectory_work_bytes)")
    _refused(lib, _fit(lib, need=0), "work buffer too small (df3d_trajectory_work_bytes)")
    for name, shown in (("pts", "pts_px"), ("X0", "X0"), ("X", "X"), ("status", "status"), ("weight", "weight"), ("err", "error"),
                        ("iterations", "iterations"), ("cost", "cost"), ("counts", "counts"), ("work", "work")):
        _refused(lib, _fit(lib, **{name: None}), f"null pointer: {shown}")
    _refused(lib, _fit(lib, pts=A + 4), "pts_px must be 8-byte aligned")
    _refused(lib, _fit(lib, iterations=A + 6 * STEP + 2), "iterations must be 4-byte aligned")
    _refused(lib, _fit(lib, counts=A + 8 * STEP + 4), "counts must be 8-byte aligned")
    _refused(lib, _fit(lib, work=A + 9 * STEP + 4), "work must be 8-byte aligned")
    _refused(lib, _fit(lib, X=A + STEP + T * J * 24 - 8), "X must not overlap X0")          # the fit is not in place
    _refused(lib, _fit(lib, X0=A + NCAM * T * J * 16 - 8), "X0 must not overlap pts_px")
    _refused(lib, _fit(lib, err=A + 4 * STEP + NCAM * T * J * 8 - 8), "error must not overlap weight")
    _refused(lib, _fit(lib, cost=A + 6 * STEP), "cost must not overlap iterations")
    _refused(lib, _fit(lib, work=A + 8 * STEP + J * 40 - 8), "work must not overlap counts")


def test_linearize_refusals(native_lib):
    lib = native_lib
    _refused(lib, _linearize(lib, ncam=9), "ncam must be in [1, 8]", LIN)
    _refused(lib, _linearize(lib, J=65), "J must be in [1, 64]", LIN)
    _refused(lib, _linearize(lib, T=-1), "T must be in [0, 1048576]", LIN)
    for bad in (NAN, -1.0):
        _refused(lib, _linearize(lib, delta=bad), "delta must be >= 0 and not NaN", LIN)
    _refused(lib, _linearize(lib, P=None), "null pointer: P_host", LIN)
    _refused(lib, _linearize(lib, need=T * J * 8 - 1), "work buffer too small", LIN)
    for name, shown in (("pts", "pts_px"), ("X", "X"), ("H", "H"), ("g", "g"), ("weight", "weight"), ("err", "err"), ("cost", "cost"),
                        ("work", "work")):
        _refused(lib, _linearize(lib, **{name: None}), f"null pointer: {shown}", LIN)
    _refused(lib, _linearize(lib, H=A + 2 * STEP + 4), "H must be 8-byte aligned", LIN)
    _refused(lib, _linearize(lib, g=A + 2 * STEP + T * J * 48 - 8), "g must not overlap H", LIN)
    _refused(lib, _linearize(lib, cost=A + 7 * STEP), "work must not overlap cost", LIN)
    assert _linearize(lib, T=0, P=None, pts=None, X=None, H=None, g=None, weight=None, err=None, cost=None, work=None, need=0, delta=INF) == 0


def test_solve_refusals(native_lib):
    lib = native_lib
    _refused(lib, _solve(lib, J=0, need=1 << 40), "J must be in [1, 64]", SOLVE)
    _refused(lib, _solve(lib, T=-1, need=1 << 40), "T must be in [0, 1048576]", SOLVE)
    for block in (2, (1 << 20) + 1):
        _refused(lib, _solve(lib, B=block), "block_frames must be in [3, 1048576]", SOLVE)
    for bad in (NAN, -1e-3, 1e14):
        _refused(lib, _solve(lib, mu=bad), "mu must be in [0, 1e13]", SOLVE)
    for bad in (NAN, -1.0, INF):
        _refused(lib, _solve(lib, lam=_doubles([bad] * 64)), "lambda must be >= 0 and finite", SOLVE)
    _refused(lib, _solve(lib, lam=None), "null pointer: lambda_host", SOLVE)
    _refused(lib, _solve(lib, need=8), "work buffer too small (df3d_trajectory_work_bytes)", SOLVE)
    for name in ("H", "g", "segment", "d", "ok", "work"):
        _refused(lib, _solve(lib, **{name: None}), f"null pointer: {name}", SOLVE)
    _refused(lib, _solve(lib, ok=A + 4 * STEP + 2), "ok must be 4-byte aligned", SOLVE)
    _refused(lib, _solve(lib, d=A + STEP + T * J * 24 - 8), "d must not overlap g", SOLVE)
    _refused(lib, _solve(lib, d=A + 2 * STEP + T * J - 1 - (T * J - 1) % 8), "d must not overlap segment", SOLVE)
    _refused(lib, _solve(lib, ticks=A + 6 * STEP + 4), "ticks must be 8-byte aligned", SOLVE)
    _refused(lib, _solve(lib, ticks=A + 4 * STEP), "ticks must not overlap ok", SOLVE)
    assert _solve(lib, T=0, H=None, g=None, segment=None, d=None, ok=None, work=None, ticks=None, need=0, lam=None) == 0


def test_no_frames_succeed(native_lib):
    lib = native_lib
    none = (None,) * 8
    assert lib.df3d_triangulate_trajectory(None, None, None, NCAM, 0, J, None, 10.0, 10, B, *none, 0, None) == 0
    # ... but the parameters are still checked
    _refused(lib, lib.df3d_triangulate_trajectory(None, None, None, 9, 0, J, None, 10.0, 10, B, *none, 0, None), "ncam must be")
    _refused(lib, lib.df3d_triangulate_trajectory(None, None, None, NCAM, 0, J, None, NAN, 10, B, *none, 0, None), "delta must be")
    _refused(lib, lib.df3d_triangulate_trajectory(None, None, None, NCAM, 0, J, None, 10.0, -1, B, *none, 0, None), "max_gap must be")
    _refused(lib, lib.df3d_triangulate_trajectory(None, None, None, NCAM, 0, J, None, 10.0, 10, 2, *none, 0, None), "block_frames must be")
    _refused(lib, _fit(lib, T=0, lam=_doubles([NAN] * 64)), "lambda must be")


def test_the_entries_are_exported_and_the_abi_stays(native_lib):
    from deepfly3d_amd import _native

    for name in NAMES:
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == _native.ABI_VERSION == 610
    assert _native.PROTOTYPES["df3d_trajectory_work_bytes"] == (ctypes.c_longlong, [ctypes.c_int] * 4)
    text = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    assert re.search(r"#define\s+DF3D_ABI_VERSION\s+610\b", text) and "a20 trajectory triangulation" in text
    assert text.index("a19 consensus triangulation") < text.index("a20 trajectory triangulation")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        declared = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code)
        assert declared and len(declared.group(1).split(",")) == len(_native.PROTOTYPES[name][1]), name
    flags = open(os.path.join(ROOT, "deepfly3d_amd", "build.py")).read()
    assert '"trajectory.hip": ["-ffp-contract=off"]' in flags
