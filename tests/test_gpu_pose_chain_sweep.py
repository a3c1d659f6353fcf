"""-m gpu sweep of the 3-D pose chain's kernels (csrc/geometry.hip, csrc/geometry_dev.h, csrc/pose3d.hip) over routes, shapes and edge
inputs, on the seeded cases of tests/pose_chain_cases.py, against the float64 oracles (oracle/geometry.py, oracle/postprocess.py) and
numpy.median.  tests/test_pose_chain_cases_host.py proves on the CPU what each bar rests on (see the case module's docstring); nothing
here skips or weakens at run time.

Every call under test goes through the C ABI into a buffer that is filled with one NaN bit pattern and has guard words of the same pattern
behind it (`_Out`): an element no thread wrote, or a write past the end, fails the test.  Where deepfly3d_amd.ops exposes the same form of
the call, the ops call is made as well and must return the same bits."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import pose_chain_cases as pc
from oracle import postprocess as pp

pytestmark = pytest.mark.gpu

PATTERN = 0x7FF80BAD0BAD0BAD     # a quiet NaN no arithmetic produces
GUARD = 16
DP = ctypes.POINTER(ctypes.c_double)


class _Out:
    """n doubles of PATTERN on the device with GUARD more behind them."""

    def __init__(self, shape, cuda, guard=GUARD):
        self.shape, self.n = tuple(shape), int(np.prod(shape, dtype=np.int64))
        self.buf = torch.full((self.n + guard,), PATTERN, dtype=torch.int64, device=cuda)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def bits(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[self.n :] == PATTERN).all(), "a write behind the end of the buffer"
        return b[: self.n]

    def get(self):
        b = self.bits()
        assert not (b == PATTERN).any(), "%d elements were not written" % int((b == PATTERN).sum())
        return b.view(np.float64).reshape(self.shape)

    def untouched(self):
        return bool((self.bits() == PATTERN).all())


def _up(a, cuda):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(cuda)   # (a copy: the cached cases are read-only)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def env(native_lib, cuda):
    from deepfly3d_amd import _native, ops

    return native_lib, cuda, _native, ops


# ---------------------------------------------------------------- re-layout (bit-exact) ----------------------------------------------
def _relayout(env, p, ordering, check_ops=True):
    lib, cuda, _native, ops = env
    T = p.shape[1]
    x = _up(p, cuda)
    out = _Out((7, T, 38, 2), cuda)
    _native.check(lib.df3d_relayout_19_to_38(x.data_ptr(), (ctypes.c_int * 7)(*ordering), T, out.ptr, _stream()), "df3d_relayout_19_to_38")
    got = out.get()
    if check_ops:
        assert _same(ops.relayout_19_to_38(x, ordering).cpu().numpy(), got)
    return got


def test_relayout_all_orderings(env):
    from oracle import geometry as og

    lib, cuda, _native, ops = env
    p = pc.relayout_input(2)
    x = _up(p, cuda)                                                   # one upload
    n, stride = 7 * 2 * 38 * 2, 7 * 2 * 38 * 2 + GUARD
    buf = torch.full((len(pc.ORDERINGS), stride), PATTERN, dtype=torch.int64, device=cuda)   # every call's output with its own guard words
    via_ops = []
    for i, o in enumerate(pc.ORDERINGS):
        _native.check(lib.df3d_relayout_19_to_38(x.data_ptr(), (ctypes.c_int * 7)(*o), 2, buf.data_ptr() + 8 * stride * i, _stream()), "df3d_relayout_19_to_38")
        via_ops.append(ops.relayout_19_to_38(x, o))
    torch.cuda.synchronize()
    bits = buf.cpu().numpy()
    via_ops = torch.stack(via_ops).cpu().numpy()
    assert (bits[:, n:] == PATTERN).all() and not (bits[:, :n] == PATTERN).any()
    got = np.ascontiguousarray(bits[:, :n]).view(np.float64).reshape(len(pc.ORDERINGS), 7, 2, 38, 2)
    want = np.stack([og.relayout_19_to_38(p, o) for o in pc.ORDERINGS])
    wrong = [o for o, g, w in zip(pc.ORDERINGS, got, want) if not np.array_equal(g, w)]
    assert not wrong, "%d orderings differ from the oracle, the first %s" % (len(wrong), wrong[0])
    assert np.array_equal(via_ops, want)


@pytest.mark.parametrize("T", pc.RELAYOUT_EDGE_T)
def test_relayout_block_edges(env, T):
    from oracle import geometry as og

    p = pc.relayout_input(T, seed=T)
    for o in (tuple(range(7)), tuple(range(6, -1, -1))):
        assert np.array_equal(_relayout(env, p, o), og.relayout_19_to_38(p, o))


def test_relayout_passes_non_finite_values_through(env):
    from oracle import geometry as og

    p = pc.relayout_input(3, seed=9)
    p[1, 0, 4] = (np.nan, 0.25)          # a NaN row of a right camera
    p[5, 1, 7] = (0.5, np.nan)           # a NaN column of a left camera: 1 - NaN
    p[2, 2, 3] = (np.inf, 0.75)
    p[6, 0, 18] = (0.125, -np.inf)       # 1 - (-inf) = inf
    for o in (tuple(range(7)), (3, 5, 1, 0, 2, 6, 4)):
        want = og.relayout_19_to_38(p, o)
        got = _relayout(env, p, o)
        assert np.isnan(want).sum() >= 1 and np.isinf(want).sum() >= 1
        assert np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------- triangulation ------------------------------------------------------
def _triangulate(env, P, px, scales=None, device_P=False, check_ops=True):
    """df3d_triangulate (or _scaled with scales = (row, col)) of px [ncam, T, J, 2] (numpy or device tensor) into a guarded buffer."""
    lib, cuda, _native, ops = env
    x = px if isinstance(px, torch.Tensor) else _up(px, cuda)
    ncam, T, J, _ = x.shape
    Ph = np.ascontiguousarray(P[:ncam], dtype=np.float64)
    Pd = _up(Ph, cuda) if device_P else None
    Pptr = Pd.data_ptr() if device_P else Ph.ctypes.data
    out = _Out((T, J, 3), cuda)
    if scales is None:
        _native.check(lib.df3d_triangulate(Pptr, x.data_ptr(), ncam, T, J, out.ptr, _stream()), "df3d_triangulate")
    else:
        _native.check(lib.df3d_triangulate_scaled(Pptr, x.data_ptr(), scales[0], scales[1], ncam, T, J, out.ptr, _stream()), "df3d_triangulate_scaled")
    got = out.get()
    if check_ops and scales is None and not device_P:
        assert _same(ops.triangulate(Ph, x).cpu().numpy(), got)
    return got


def test_triangulate_camera_subsets_against_the_svd_oracle(env):
    P, _ = pc.rig()
    px = pc.detections()[0]
    worst = {}
    for cams in pc.TRI_SUBSETS:
        got = _triangulate(env, P, pc.only_cameras(px, cams))
        e = np.abs(got - pc.tri_oracle(cams)).max()
        if not e < worst.get(len(cams), (-1.0, None))[0]:
            worst[len(cams)] = (e, cams)
    for k, (e, cams) in worst.items():
        print("triangulation, %d cameras: worst |device - SVD oracle| %.2e mm at %s (bar %.0e)" % (k, e, cams, pc.TRI_BAR))
    assert all(e < pc.TRI_BAR for e, _ in worst.values())


@pytest.fixture(scope="module")
def mixed_views(env):
    """1520 points, each seen by one of the sweep's camera subsets in turn, as a T = 40, J = 38 call: (px [8, 40, 38, 2], its result)."""
    px = pc.detections(seed=12, npoints=40 * 38)[0].copy()
    for q in range(px.shape[1]):
        keep = np.zeros(8, dtype=bool)
        keep[list(pc.TRI_SUBSETS[q % len(pc.TRI_SUBSETS)])] = True
        px[~keep, q] = 0.0
    px = px.reshape(8, 40, 38, 2)
    return px, _triangulate(env, pc.rig()[0], px)


def test_triangulate_a_point_does_not_depend_on_its_batch(env, mixed_views):
    lib, cuda, _native, ops = env
    P, _ = pc.rig()
    px, full = mixed_views
    flat, full = px.reshape(8, 1520, 1, 2), full.reshape(1520, 3)
    fixed = [0, 1, 37, 38, 255, 256, 257, 511, 512, 1023, 1024, 1519]            # block and frame edges of the big call, then 28 seeded others
    picks = fixed + [q for q in np.random.default_rng(3).permutation(1520).tolist() if q not in fixed][:28]
    assert len(picks) == 40
    filler = _up(flat[:, 600:857].copy(), cuda)                      # a 257-point launch: 256 others and the point as the last element, the
    for q in picks:                                                   # only thread of the second block
        alone = _triangulate(env, P, flat[:, q : q + 1], check_ops=False)
        assert _same(alone[0, 0], full[q]), q
        filler[:, 256] = _up(flat[:, q], cuda)
        last = _triangulate(env, P, filler, check_ops=False)
        assert _same(last[256, 0], full[q]), q


def test_triangulate_camera_count_equals_zeroed_cameras(env):
    P, _ = pc.rig()
    px = pc.detections()[0]
    for k in range(1, 8):
        few = _triangulate(env, P, px[:k].copy())                                   # ncam = k
        zeroed = _triangulate(env, P, pc.only_cameras(px, range(k)))                # ncam = 8
        assert _same(few, zeroed), k
        if k == 1:
            assert not few.any() and not np.signbit(few).any()                      # one view: exactly +0.0
        else:
            assert np.abs(few - pc.detections()[1][:, None]).max() < 5.0


def test_triangulate_scaled_and_device_resident_cameras(env):
    lib, cuda, _native, ops = env
    P, _ = pc.rig()
    px = pc.detections()[0]
    H, W = 480.0, 960.0
    norm = px / np.array([H, W])
    plain = _triangulate(env, P, norm * np.array([H, W]))
    assert _same(_triangulate(env, P, norm, scales=(H, W)), plain)
    assert _same(_triangulate(env, P, norm, scales=(H, W), device_P=True), plain)
    want = _triangulate(env, P, px)
    assert _same(_triangulate(env, P, px, device_P=True), want)
    for k in (1, 2, 7):                                                             # the device copy moves 12 * ncam doubles, not 96
        assert _same(_triangulate(env, P, px[:k].copy(), device_P=True), _triangulate(env, P, px[:k].copy()))


def test_triangulate_visibility_rule(env):
    from oracle import geometry as og

    P, _ = pc.rig()
    px = pc.visibility_case()
    got = _triangulate(env, P, px)[:, 0]
    ref = og.triangulate_dlt(px, P)[:, 0]
    assert not got[1].any() and not got[3].any() and not np.signbit(got[[1, 3]]).any()      # no view, one view: exactly 0.0
    assert got[0].all() and np.abs(got[0] - ref[0]).max() < pc.TRI_BAR                       # exactly two views: solved
    assert _same(got[2], _triangulate(env, P, pc.only_cameras(px, range(2, 8)))[2, 0])       # -0.0 in either coordinate: not seen
    assert np.abs(got[2] - ref[2]).max() < pc.TRI_BAR


def test_triangulate_nan_detection_stays_in_its_point(env):
    P, _ = pc.rig()
    clean = pc.detections()[0]
    px = clean.copy()
    px[3, 77, 0, 0] = np.nan         # a row
    px[0, 256, 0, 1] = np.nan        # a column, first thread of the second block
    px[7, 299, 0, :] = np.nan        # both, the last point
    want, got = _triangulate(env, P, clean), _triangulate(env, P, px)
    bad = np.zeros(300, dtype=bool)
    bad[[77, 256, 299]] = True
    assert not np.isfinite(got[bad]).any()
    assert _same(got[~bad], want[~bad])


def test_triangulate_bad_arguments(env):
    lib, cuda, _native, ops = env
    P, _ = pc.rig()
    x = _up(pc.detections()[0][:, :4], cuda)
    out = _Out((4, 1, 3), cuda)
    Pp, s = P.ctypes.data, _stream()
    bad = [
        lib.df3d_triangulate(Pp, x.data_ptr(), 0, 4, 1, out.ptr, s),
        lib.df3d_triangulate(Pp, x.data_ptr(), 9, 4, 1, out.ptr, s),
        lib.df3d_triangulate(Pp, x.data_ptr(), 8, 4, 0, out.ptr, s),
        lib.df3d_triangulate(Pp, x.data_ptr(), 8, -1, 1, out.ptr, s),
        lib.df3d_triangulate(None, x.data_ptr(), 8, 4, 1, out.ptr, s),
        lib.df3d_triangulate(Pp, None, 8, 4, 1, out.ptr, s),
        lib.df3d_triangulate(Pp, x.data_ptr(), 8, 4, 1, None, s),
        lib.df3d_triangulate_scaled(Pp, x.data_ptr(), 0.0, 1.0, 8, 4, 1, out.ptr, s),
        lib.df3d_triangulate_scaled(Pp, x.data_ptr(), 1.0, -2.0, 8, 4, 1, out.ptr, s),
        lib.df3d_triangulate_scaled(Pp, x.data_ptr(), 1.0, 1.0, 8, 4, 0, out.ptr, s),
    ]
    assert bad == [_native.DF3D_EINVAL] * len(bad)
    assert lib.df3d_triangulate(None, None, 8, 0, 1, None, s) == 0                  # no frames: nothing to read or write
    assert lib.df3d_triangulate_scaled(None, None, 2.0, 3.0, 1, 0, 38, None, s) == 0
    assert out.untouched()                                                           # none of them launched
    with pytest.raises(_native.NativeLibraryError):
        _native.check(lib.df3d_triangulate(Pp, x.data_ptr(), 9, 4, 1, out.ptr, s), "df3d_triangulate")


# ---------------------------------------------------------------- medians (bit-exact against numpy.median) ---------------------------
@pytest.mark.parametrize("n", pc.COLUMN_MEDIAN_N)
def test_column_median_with_padded_columns(env, n):
    lib, cuda, _native, ops = env
    cols = np.stack([pc.median_column(k, n) for k in pc.COLUMN_KINDS])
    padded = np.empty((len(cols), n + 3))
    padded[:, :n] = cols
    padded[0::2, n:] = 1.7e308               # behind every column three huge values that are not part of it
    padded[1::2, n:] = -1.7e308
    out = _Out((len(cols),), cuda)
    _native.check(lib.df3d_column_median(_up(padded, cuda).data_ptr(), len(cols), n, n + 3, out.ptr, _stream()), "df3d_column_median")
    want = np.median(cols, axis=1)
    assert np.isfinite(want).all()
    assert np.array_equal(out.get(), want)
    assert np.array_equal(ops.column_median(_up(cols, cuda)).cpu().numpy(), want)


def _normalize(env, x, work_len):
    lib, cuda, _native, ops = env
    T, J, _ = x.shape
    out, work = _Out((T, J, 3), cuda), _Out((work_len,), cuda)
    _native.check(lib.df3d_pose_normalize(x.data_ptr(), T, J, 0, out.ptr, work.ptr, work_len, _stream()), "df3d_pose_normalize")
    work.bits()                              # (the guard words behind the scratch of the long route)
    return out.get()


@pytest.mark.parametrize("T,J", pc.NORMALIZE_SHAPES)
def test_pose_normalize_at_the_route_switch(env, T, J):
    lib, cuda, _native, ops = env
    for run in pc.median_runs(T * J, seed=J):
        X = run.reshape(T, J, 3)
        x = _up(X, cuda)
        want = X - np.median(run, axis=0)
        got = ops.pose_normalize(x, rotate=False).cpu().numpy()
        assert np.array_equal(got, want)
        for work_len in (3, pc.MED_LONG_WORK - 1, pc.MED_LONG_WORK, 1024):   # one workgroup per column up to 823, the long route from 824
            assert _same(_normalize(env, x, work_len), got), work_len


def test_pose_normalize_bad_arguments(env):
    lib, cuda, _native, ops = env
    x = _up(np.zeros((4, 2, 3)), cuda)
    out, work, s = _Out((4, 2, 3), cuda), _Out((8,), cuda), _stream()
    bad = [
        lib.df3d_pose_normalize(x.data_ptr(), 4, 2, 0, out.ptr, work.ptr, 2, s),
        lib.df3d_pose_normalize(x.data_ptr(), 0, 2, 0, out.ptr, work.ptr, 8, s),
        lib.df3d_pose_normalize(x.data_ptr(), 4, 0, 0, out.ptr, work.ptr, 8, s),
        lib.df3d_pose_normalize(None, 4, 2, 0, out.ptr, work.ptr, 8, s),
        lib.df3d_pose_normalize(x.data_ptr(), 4, 2, 0, out.ptr, None, 8, s),
    ]
    assert bad == [_native.DF3D_EINVAL] * len(bad) and out.untouched() and work.untouched()


# ---------------------------------------------------------------- Procrustes ---------------------------------------------------------
def _constants(name):
    from deepfly3d_amd.procrustes import template_constants

    return template_constants(pc.templates()[name])


def _procrustes(env, X, consts, check_ops=True):
    lib, cuda, _native, ops = env
    seg, fit = (np.ascontiguousarray(c, dtype=np.float64) for c in consts)
    x = _up(X, cuda)
    T = X.shape[0]
    need = lib.df3d_procrustes_work_doubles(T)
    out, work = _Out(X.shape, cuda), _Out((need,), cuda)
    _native.check(lib.df3d_procrustes(x.data_ptr(), T, seg.ctypes.data_as(DP), fit.ctypes.data_as(DP), out.ptr, work.ptr, need, _stream()), "df3d_procrustes")
    work.bits()
    got = out.get()
    if check_ops:
        assert _same(ops.procrustes(x, seg, fit).cpu().numpy(), got)
    return got


@pytest.mark.parametrize("T", pc.PROCRUSTES_T)
@pytest.mark.parametrize("name", ["default", "golden"])
def test_procrustes_rigid_motions_against_the_oracle(env, name, T):
    from oracle import geometry as og

    tmpl, consts, worst = pc.templates()[name], _constants(name), 0.0
    for draw in range(pc.PROCRUSTES_DRAWS):
        X = pc.moved_pose(T, draw)
        e = np.abs(_procrustes(env, X, consts) - og.procrustes_separate(X, tmpl)).max()
        worst = e if not e < worst else worst
    print("Procrustes, %s template, T = %d: worst |device - oracle| %.2e over %d draws (bar %.0e)" % (name, T, worst, pc.PROCRUSTES_DRAWS, pc.PROCRUSTES_BAR))
    assert worst < pc.PROCRUSTES_BAR


@pytest.mark.parametrize("T", pc.PROCRUSTES_SWITCH_T)
def test_procrustes_at_the_median_route_switch(env, T):
    from oracle import geometry as og

    X = pc.long_pose(T)
    e = np.abs(_procrustes(env, X, _constants("golden")) - og.procrustes_separate(X, pc.templates()["golden"])).max()
    print("Procrustes, T = %d: |device - oracle| %.2e (bar %.0e)" % (T, e, pc.PROCRUSTES_BAR))
    assert e < pc.PROCRUSTES_BAR


@pytest.mark.parametrize("T", [15, 3450])
def test_procrustes_does_not_depend_on_the_frame_order(env, T):
    """Every sequence-global quantity is an exact order statistic and every frame is mapped on its own: permuting the frames permutes
    the output, bit for bit -- at 3450 frames through the strided medians of the multi-workgroup route."""
    X = pc.long_pose(T) if T > 15 else pc.moved_pose(15, 1)
    perm = np.random.default_rng(T).permutation(T)
    consts = _constants("golden")
    assert _same(_procrustes(env, X[perm], consts), _procrustes(env, X, consts)[perm])


@pytest.mark.parametrize("side", [0, 1])
def test_procrustes_sides_are_independent_and_a_lost_side_is_nan(env, side):
    keep, other = pc.SIDES[side], pc.SIDES[1 - side]
    consts = _constants("default")
    X = pc.golden_pose()
    base = _procrustes(env, X, consts)
    assert np.isfinite(base).all()
    assert np.abs(base - pc.oracle_procrustes(X, pc.templates()["default"])).max() < pc.PROCRUSTES_BAR
    Y = X.copy()
    Y[:, other] = pc.moved_pose(15, 4)[:, other]           # other finite data on the other side
    assert _same(_procrustes(env, Y, consts)[:, keep], base[:, keep])
    for Z in (pc.zero_side_pose(1 - side), pc.zero_legs_pose(1 - side)):   # the other side lost: NaN there, this side untouched
        got = _procrustes(env, Z, consts)
        assert np.isnan(got[:, other]).all()
        assert _same(got[:, keep], base[:, keep])


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("case", ["coplanar", "collinear"])
def test_procrustes_degenerate_fit_by_property(env, case, side):
    """Rank 2 (coplanar fit joints: the `weak` branch of rigid_fit_kernel) and rank 1 (collinear: two weak columns).  The reference's SVD
    is arbitrary in the null directions, so: the side's map is a rigid one, the output is finite, the six median fit joints land where the
    oracle puts them (on their span the minimiser is unique), and a second call returns the same bits.
    Before rigid_fit_kernel completed U for rank 1 the collinear case read an undefined column of it: the side came out non-finite (both
    sides tried: |R^T R - I| = 1, the fit joints 2.4 and 3.2 mm from the oracle's), the coplanar case as it is now."""
    sl, consts, tmpl = pc.SIDES[side], _constants("default"), pc.templates()["default"]
    X = pc.degenerate_pose(case, side)
    got = _procrustes(env, X, consts)
    again = _procrustes(env, X, consts)
    f = pc.side_fit(X[:, sl], tmpl[:, sl])
    src, dst = X[:, sl].reshape(-1, 3), got[:, sl].reshape(-1, 3)
    finite = bool(np.isfinite(got).all())
    A = np.concatenate([src, np.ones((len(src), 1))], axis=1)
    sol = np.linalg.lstsq(A, np.nan_to_num(dst), rcond=None)[0]
    M, c = sol[:3], sol[3]
    affine = np.abs(A @ sol - dst).max()
    R = M / f["s"]
    ortho = np.abs(R.T @ R - np.eye(3)).max()
    fit_in = np.median(X[:, sl][:, list(pc.FIT_JOINTS)], axis=0)
    e_fit = np.abs(fit_in @ M + c - (f["Y"] @ f["Tm"] + f["c"])).max()
    print("%s, side %d: finite %s  |affine residual| %.2e  |R^T R - I| %.2e (bar 1e-12)  fit joints vs oracle %.2e (bar %.0e)  same bits twice %s"
          % (case, side, finite, affine, ortho, e_fit, pc.PROCRUSTES_BAR, _same(got, again)))
    assert finite
    assert affine < 1e-12 and ortho < 1e-12
    assert e_fit < pc.PROCRUSTES_BAR
    assert _same(got, again)
    other = pc.SIDES[1 - side]                               # the full-rank side of the same call
    assert np.abs(got[:, other] - pc.oracle_procrustes(X, tmpl)[:, other]).max() < pc.PROCRUSTES_BAR


def test_procrustes_bad_arguments(env):
    lib, cuda, _native, ops = env
    seg, fit = (np.ascontiguousarray(c, dtype=np.float64) for c in _constants("default"))
    x = _up(pc.golden_pose(), cuda)
    need = lib.df3d_procrustes_work_doubles(15)
    assert need == 2 * (12 + 18) * 15 + 128 + 6 * 272 and lib.df3d_procrustes_work_doubles(-1) == 0
    out, work, s = _Out((15, 38, 3), cuda), _Out((need,), cuda), _stream()
    segp, fitp = seg.ctypes.data_as(DP), fit.ctypes.data_as(DP)
    bad = [
        lib.df3d_procrustes(x.data_ptr(), 15, segp, fitp, out.ptr, work.ptr, need - 1, s),
        lib.df3d_procrustes(x.data_ptr(), 0, segp, fitp, out.ptr, work.ptr, need, s),
        lib.df3d_procrustes(x.data_ptr(), 15, None, fitp, out.ptr, work.ptr, need, s),
        lib.df3d_procrustes(x.data_ptr(), 15, segp, None, out.ptr, work.ptr, need, s),
        lib.df3d_procrustes(None, 15, segp, fitp, out.ptr, work.ptr, need, s),
    ]
    assert bad == [_native.DF3D_EINVAL] * len(bad) and out.untouched() and work.untouched()


# ---------------------------------------------------------------- One-Euro (bit-exact, default stamps) -------------------------------
@pytest.mark.parametrize("T,nch", list(itertools.product(pc.ONEEURO_T, pc.ONEEURO_NCH)))
def test_oneeuro_short_series_and_block_edges(env, T, nch):
    lib, cuda, _native, ops = env
    X = pc.oneeuro_input(T, nch)
    x = _up(X, cuda)
    want = pp.oneeuro_filter(X)
    out = _Out((T, nch), cuda)
    _native.check(lib.df3d_oneeuro_filter(x.data_ptr(), T, nch, 100.0, 0.1, 2.0, 1.0, 1, 0.1, out.ptr, _stream()), "df3d_oneeuro_filter")
    assert np.array_equal(out.get(), want)
    assert np.array_equal(ops.oneeuro_filter(x).cpu().numpy(), want)
