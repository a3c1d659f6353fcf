"""CPU tests of the three C entries of the consensus triangulation (include/df3d_hip.h, a19): every refusal comes before the device is
touched and carries a message, so these run without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 28   # addresses that are never dereferenced: 64-byte aligned, far from one another
STEP = 1 << 28
NCAM, T, J = 7, 100, 38
INF, NAN = float("inf"), float("nan")
NAMES = ("df3d_consensus_work_bytes", "df3d_consensus_candidates", "df3d_triangulate_consensus")
DP = ctypes.POINTER(ctypes.c_double)


def _refused(lib, rc, fragment, entry="df3d_triangulate_consensus"):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message and message.startswith(entry + ": "), (rc, message)


def _doubles(values):
    return (ctypes.c_double * len(values))(*values)


def _call(lib, **kw):
    names = ("pts", "full", "X", "cameras", "status", "err", "fixed", "counts", "work")
    a = dict(P=_doubles([1.0] * 96), ncam=NCAM, T=T, J=J, tau=_doubles([20.0] * 64), min_views=2)
    a.update({n: A + k * STEP for k, n in enumerate(names)})
    a.update(kw)
    if "need" not in a:
        a["need"] = max(lib.df3d_consensus_work_bytes(a["ncam"], a["T"], a["J"]), 0)
    P = a["P"] if a["P"] is None else ctypes.cast(a["P"], DP)
    tau = a["tau"] if a["tau"] is None else ctypes.cast(a["tau"], DP)
    return lib.df3d_triangulate_consensus(P, a["pts"], a["full"], a["ncam"], a["T"], a["J"], tau, a["min_views"], a["X"], a["cameras"], a["status"],
                                          a["err"], a["fixed"], a["counts"], a["work"], a["need"], None)


def _candidates(lib, **kw):
    a = dict(P=_doubles([1.0] * 96), pts=A, full=A + STEP, ncam=3, T=T, J=J, cand_X=A + 2 * STEP, cand_q=A + 3 * STEP)
    a.update(kw)
    P = a["P"] if a["P"] is None else ctypes.cast(a["P"], DP)
    return lib.df3d_consensus_candidates(P, a["pts"], a["full"], a["ncam"], a["T"], a["J"], a["cand_X"], a["cand_q"], None)


def test_work_bytes(native_lib):
    lib = native_lib
    for bad in ((0, T, J), (9, T, J), (NCAM, -1, J), (NCAM, T, 0), (NCAM, T, 65)):
        assert lib.df3d_consensus_work_bytes(*bad) == 0, bad
    for frames in (1, 255, 256, 257, 1000, 100000):
        need = lib.df3d_consensus_work_bytes(NCAM, frames, J)
        exact = -(-frames // 256) * J * 4 * 8   # [slices of 256 frames, J, 4] int64
        assert need % 64 == 0 and exact <= need < exact + 64, frames
    assert lib.df3d_consensus_work_bytes(NCAM, 0, J) == 0
    assert lib.df3d_consensus_work_bytes(1, T, J) == lib.df3d_consensus_work_bytes(8, T, J)


def test_refusals(native_lib):
    lib = native_lib
    for ncam in (0, 9, -1):
        _refused(lib, _call(lib, ncam=ncam, need=1 << 30), "ncam must be in [1, 8]")
    for j in (0, 65):
        _refused(lib, _call(lib, J=j, need=1 << 30), "J must be in [1, 64]")
    _refused(lib, _call(lib, T=-1, need=1 << 30), "T must be >= 0")
    for m in (1, 0, 9, -2):
        _refused(lib, _call(lib, min_views=m), "min_views must be in [2, 8]")
    for bad in (NAN, -1.0, -INF):
        _refused(lib, _call(lib, tau=_doubles([20.0] * 37 + [bad] + [20.0] * 26)), "tau must be >= 0 and not NaN")
    assert _call(lib, T=0, tau=_doubles([INF, 0.0] * 32)) == 0   # +inf and 0 are values
    _refused(lib, _call(lib, P=None), "null pointer: P_host")
    _refused(lib, _call(lib, tau=None), "null pointer: tau_host")
    need = lib.df3d_consensus_work_bytes(NCAM, T, J)
    _refused(lib, _call(lib, need=need - 1), "work buffer too small (df3d_consensus_work_bytes)")
    _refused(lib, _call(lib, need=0), "work buffer too small (df3d_consensus_work_bytes)")
    for name, shown in (("pts", "pts_px"), ("full", "X_full"), ("X", "X"), ("cameras", "cameras"), ("status", "status"), ("err", "err"),
                        ("work", "work")):
        _refused(lib, _call(lib, **{name: None}), f"null pointer: {shown}")
    _refused(lib, _call(lib, pts=A + 4), "pts_px must be 8-byte aligned")
    _refused(lib, _call(lib, cameras=A + 3 * STEP + 2), "cameras must be 4-byte aligned")
    _refused(lib, _call(lib, counts=A + 7 * STEP + 4), "counts must be 8-byte aligned")
    _refused(lib, _call(lib, X=A + NCAM * T * J * 16 - 8), "X must not overlap pts_px")
    _refused(lib, _call(lib, X=A + STEP + T * J * 24 - 8), "X must not overlap X_full")
    _refused(lib, _call(lib, fixed=A + 5 * STEP + NCAM * T * J * 8 - 8), "fixed_px must not overlap err")
    _refused(lib, _call(lib, counts=A + 4 * STEP), "counts must not overlap status")
    _refused(lib, _call(lib, work=A + 7 * STEP + J * 32 - 8), "counts must not overlap work")


def test_candidates_refusals(native_lib):
    lib, entry = native_lib, "df3d_consensus_candidates"
    for ncam in (0, 9):
        _refused(lib, _candidates(lib, ncam=ncam), "ncam must be in [1, 8]", entry)
    _refused(lib, _candidates(lib, J=65), "J must be in [1, 64]", entry)
    _refused(lib, _candidates(lib, T=-1), "T must be >= 0", entry)
    _refused(lib, _candidates(lib, P=None), "null pointer: P_host", entry)
    for name, shown in (("pts", "pts_px"), ("full", "X_full"), ("cand_X", "cand_X"), ("cand_q", "cand_q")):
        _refused(lib, _candidates(lib, **{name: None}), f"null pointer: {shown}", entry)
    _refused(lib, _candidates(lib, cand_q=A + 2 * STEP + T * J * 8 * 24 - 8), "cand_q must not overlap cand_X", entry)
    _refused(lib, _candidates(lib, cand_X=A + 8), "cand_X must not overlap pts_px", entry)
    assert _candidates(lib, T=0, P=None, pts=None, full=None, cand_X=None, cand_q=None) == 0


def test_no_frames_succeed(native_lib):
    lib = native_lib
    assert lib.df3d_triangulate_consensus(None, None, None, NCAM, 0, J, None, 2, None, None, None, None, None, None, None, 0, None) == 0
    # ... but the parameters are still checked
    _refused(lib, lib.df3d_triangulate_consensus(None, None, None, 9, 0, J, None, 2, None, None, None, None, None, None, None, 0, None), "ncam must be")
    _refused(lib, lib.df3d_triangulate_consensus(None, None, None, NCAM, 0, J, None, 1, None, None, None, None, None, None, None, 0, None), "min_views must be")
    _refused(lib, _call(lib, T=0, tau=_doubles([NAN] * 64)), "tau must be")


def test_the_entries_are_exported_and_the_abi_stays(native_lib):
    from deepfly3d_amd import _native

    for name in NAMES:
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == _native.ABI_VERSION == 610
    assert _native.PROTOTYPES["df3d_consensus_work_bytes"] == (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int, ctypes.c_int])
    text = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    assert re.search(r"#define\s+DF3D_ABI_VERSION\s+610\b", text) and "a19 consensus triangulation over camera subsets" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        declared = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code)
        assert declared and len(declared.group(1).split(",")) == len(_native.PROTOTYPES[name][1]), name
    flags = open(os.path.join(ROOT, "deepfly3d_amd", "build.py")).read()
    assert '"consensus.hip": ["-ffp-contract=off"]' in flags
