"""CPU tests of the three C entries of the heat-map triangulation (include/df3d_hip.h, a21): every refusal comes before the device is
touched and carries a message, so these run without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 32   # addresses that are never dereferenced: 64-byte aligned, far from one another
STEP = 1 << 32
N, V, C, H, W, J, M, LEVELS = 2, 6, 19, 64, 128, 38, 5, 4
INF, NAN = float("inf"), float("nan")
SCORES, SEARCH = "df3d_heatmap3d_scores", "df3d_triangulate_heatmaps"
NAMES = ("df3d_heatmap3d_window_doubles", SCORES, SEARCH)
DP, BP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)


def _refused(lib, rc, fragment, entry=SEARCH):
    message = lib.df3d_last_error().decode()
    assert rc == -1 and fragment in message and message.startswith(entry + ": "), (rc, message)


def _host(a):
    return dict(P=(ctypes.c_double * 96)(*([1.0] * 96)), flip=(ctypes.c_ubyte * 8)(), plane=(ctypes.c_int * (8 * 64))(*([0] * 512)), **a)


def _cast(v, kind):
    return v if v is None else ctypes.cast(v, kind)


def _search(lib, **kw):
    names = ("hm", "X0", "X", "score", "status", "views", "shift", "choice", "counts", "path")
    a = _host(dict(n=N, V=V, C=C, H=H, W=W, J=J, half=0.4, levels=LEVELS, cell_rows=7.5, cell_cols=7.5, log_floor=-6.9, budget=4096))
    a.update({n: A + k * STEP for k, n in enumerate(names)})
    a.update(kw)
    return lib.df3d_triangulate_heatmaps(a["hm"], a["n"], a["V"], a["C"], a["H"], a["W"], _cast(a["P"], DP), _cast(a["flip"], BP),
                                         _cast(a["plane"], IP), a["J"], a["X0"], a["half"], a["levels"], a["cell_rows"], a["cell_cols"],
                                         a["log_floor"], a["budget"], a["X"], a["score"], a["status"], a["views"], a["shift"], a["choice"],
                                         a["counts"], a["path"], None)


def _scores(lib, **kw):
    names = ("hm", "pts", "out")
    a = _host(dict(n=N, V=V, C=C, H=H, W=W, J=J, M=M, cell_rows=7.5, cell_cols=7.5, log_floor=-6.9))
    a.update({n: A + k * STEP for k, n in enumerate(names)})
    a.update(kw)
    return lib.df3d_heatmap3d_scores(a["hm"], a["n"], a["V"], a["C"], a["H"], a["W"], _cast(a["P"], DP), _cast(a["flip"], BP),
                                     _cast(a["plane"], IP), a["J"], a["pts"], a["M"], a["cell_rows"], a["cell_cols"], a["log_floor"], a["out"], None)


def _planes(value, at):
    p = [0] * 512
    p[at] = value
    return (ctypes.c_int * 512)(*p)


def test_the_budget_is_exported(native_lib):
    assert native_lib.df3d_heatmap3d_window_doubles() == 4096   # 32 KiB of LDS: DESIGN.md section 25


def _shape_refusals(lib, call, entry):
    for v in (0, 9, -1):
        _refused(lib, call(lib, V=v), "V must be in [1, 8]", entry)
    for n in (-1, (1 << 20) + 1):
        _refused(lib, call(lib, n=n), "n must be in [0, 1048576]", entry)
    for c in (0, 1025):
        _refused(lib, call(lib, C=c), "C must be in [1, 1024]", entry)
    for h, w in ((3, 128), (64, 3), (0, 0), (1025, 128), (64, 1025)):
        _refused(lib, call(lib, H=h, W=w), "H and W must be in [4, 1024]", entry)
    for j in (0, 65):
        _refused(lib, call(lib, J=j), "J must be in [1, 64]", entry)
    for bad in (0.0, -7.5, NAN, INF):
        _refused(lib, call(lib, cell_rows=bad), "cell_rows and cell_cols must be finite and > 0", entry)
        _refused(lib, call(lib, cell_cols=bad), "cell_rows and cell_cols must be finite and > 0", entry)
    for bad in (0.0, 1.0, NAN, -INF, INF):
        _refused(lib, call(lib, log_floor=bad), "log_floor must be finite and < 0", entry)
    for name, shown in (("P", "P_host"), ("flip", "flip_host"), ("plane", "plane_host")):
        _refused(lib, call(lib, **{name: None}), f"null pointer: {shown}", entry)
    for bad, at in ((-2, 0), (C, 5 * J + 37), (1 << 20, 3 * J)):
        _refused(lib, call(lib, plane=_planes(bad, at)), "plane indices must be in [-1, C)", entry)
    assert call(lib, n=0, plane=_planes(-1, 0)) == 0                      # -1 and C - 1 are values
    _refused(lib, call(lib, hm=None), "null pointer: hm", entry)
    _refused(lib, call(lib, hm=A + 2), "hm must be 4-byte aligned", entry)


def test_search_refusals(native_lib):
    lib = native_lib
    _shape_refusals(lib, _search, SEARCH)
    for bad in (0, 7, -1):
        _refused(lib, _search(lib, levels=bad), "levels must be in [1, 6]")
    for bad in (0.0, -0.4, NAN, INF):
        _refused(lib, _search(lib, half=bad), "half must be finite and > 0")
    for bad in (-1, 4097):
        _refused(lib, _search(lib, budget=bad), "budget must be in [0, df3d_heatmap3d_window_doubles()]")
    for name in ("X0", "X", "score", "status", "views", "shift", "choice", "counts"):
        _refused(lib, _search(lib, **{name: None}), f"null pointer: {name}")
    _refused(lib, _search(lib, X0=A + STEP + 4), "X0 must be 8-byte aligned")
    _refused(lib, _search(lib, views=A + 5 * STEP + 2), "views must be 4-byte aligned")
    _refused(lib, _search(lib, choice=A + 7 * STEP + 2), "choice must be 4-byte aligned")
    _refused(lib, _search(lib, counts=A + 8 * STEP + 4), "counts must be 8-byte aligned")
    _refused(lib, _search(lib, X=A + STEP + N * J * 24 - 8), "X must not overlap X0")                 # the search is not in place
    _refused(lib, _search(lib, X0=A + N * V * C * H * W * 4 - 8), "X0 must not overlap hm")
    _refused(lib, _search(lib, status=A + 3 * STEP + N * J * 8 - 1), "status must not overlap score")
    _refused(lib, _search(lib, counts=A + 7 * STEP + N * J * LEVELS * 4 - 8), "counts must not overlap choice")
    _refused(lib, _search(lib, path=A + 4 * STEP + N * J - 1), "path must not overlap status")
    # n = 0 launches nothing, with or without buffers -- but the parameters are still checked
    none = dict(hm=None, X0=None, X=None, score=None, status=None, views=None, shift=None, choice=None, counts=None, path=None)
    assert _search(lib, n=0, **none) == 0 and _search(lib, n=0, P=None, flip=None, plane=None, **none) == 0
    _refused(lib, _search(lib, n=0, levels=7, **none), "levels must be")
    _refused(lib, _search(lib, n=0, half=NAN, **none), "half must be")
    _refused(lib, _search(lib, n=0, log_floor=0.5, **none), "log_floor must be")
    _refused(lib, _search(lib, n=0, V=9, **none), "V must be")


def test_scores_refusals(native_lib):
    lib = native_lib
    _shape_refusals(lib, _scores, SCORES)
    for bad in (-1, (1 << 20) + 1):
        _refused(lib, _scores(lib, M=bad), "M must be in [0, 1048576]", SCORES)
    for name in ("pts", "out"):
        _refused(lib, _scores(lib, **{name: None}), f"null pointer: {name}", SCORES)
    _refused(lib, _scores(lib, pts=A + STEP + 4), "pts must be 8-byte aligned", SCORES)
    _refused(lib, _scores(lib, out=A + STEP + N * J * M * 24 - 8), "out must not overlap pts", SCORES)
    none = dict(hm=None, pts=None, out=None)
    assert _scores(lib, n=0, **none) == 0 and _scores(lib, M=0, **none) == 0
    _refused(lib, _scores(lib, n=0, H=3, **none), "H and W must be", SCORES)


def test_the_entries_are_exported_and_the_abi_stays(native_lib):
    from deepfly3d_amd import _native

    for name in NAMES:
        assert name in _native.PROTOTYPES and hasattr(native_lib, name)
    assert native_lib.df3d_version() == _native.ABI_VERSION == 610
    text = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    assert re.search(r"#define\s+DF3D_ABI_VERSION\s+610\b", text) and "a21 heat-map triangulation" in text
    assert text.index("a20 trajectory triangulation") < text.index("a21 heat-map triangulation")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES[1:]:
        declared = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code)
        assert declared and len(declared.group(1).split(",")) == len(_native.PROTOTYPES[name][1]), name
    flags = open(os.path.join(ROOT, "deepfly3d_amd", "build.py")).read()
    assert '"heatmap3d.hip": ["-ffp-contract=off"]' in flags
