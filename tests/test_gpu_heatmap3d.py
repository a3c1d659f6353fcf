"""-m gpu tests of the heat-map triangulation (csrc/heatmap3d.hip) against tests/heatmap3d_oracle.py: the sampler
within a bar derived below, everything discrete of the search exactly wherever the oracle's two best scores lie further apart than the
logarithm's rounding, the LDS route and the plane route bit for bit, and Core and the CLI on the two golden frames."""
import ctypes
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import heatmap3d_cases as hc
import heatmap3d_oracle as ho

pytestmark = pytest.mark.gpu

# The score's bar.  A view's term is about 50 float64 operations on values |l| <= 7 (log 1e-3 = -6.9): 50 x 7 x 1.1e-16 = 4e-14.  The
# device's logarithm may differ from numpy's by an ulp, 1e-15 on a tap's share.  The projection is the oracle's operations one by one
# (no contraction), so the cells agree to the bit; were they to differ by a rounding of 1e-13 cells, a slope of at most 7 per cell would
# make 1e-12 of it.  The bar stands two orders above the largest of these.
SCORE_BAR = 1e-10
POINT_BAR = 1e-12   # mm: the points are the same sums of the same steps once the choices agree


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the cached cases are read-only


def _search(case, cuda, **kw):
    from deepfly3d_amd import heatmap3d

    return heatmap3d.triangulate_heatmaps(case["P"], _dev(case["hm"], cuda), case["flip"], case["plane"], _dev(case["X0"], cuda), hc.IMAGE_SHAPE, **kw)


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


FIELDS = hc.FIELDS


# ---------------------------------------------------------------------------------------------------------------------- the sampler
def test_scores_on_the_edges_of_the_planes(native_lib, cuda):
    """Cells that are the point's own coordinates: on the four edges exactly, just outside, inside; a flipped and an unflipped view."""
    from deepfly3d_amd import heatmap3d

    o = hc.ortho()
    got = heatmap3d.heatmap_scores(o["P"], _dev(o["hm"], cuda), o["flip"], o["plane"], _dev(o["pts"], cuda), hc.IMAGE_SHAPE).cpu().numpy()
    want = ho.scores(o["hm"], o["P"], o["flip"], o["plane"], o["pts"], hc.IMAGE_SHAPE, hc.FLOOR)
    lf = float(np.log(hc.FLOOR))
    print(f"ortho: |device - oracle| {np.abs(got - want).max():.2e} over {want.size} points, {(want == lf + lf).sum()} of them off both planes")
    assert got.shape == want.shape and np.abs(got - want).max() <= SCORE_BAR
    assert np.array_equal(got == lf + lf, want == lf + lf) and (want == lf + lf).any() and (want > lf + lf).any()


@pytest.mark.parametrize("V", [3, 8])
def test_scores_round_planted_blobs(native_lib, cuda, V):
    """Points inside the planes, far outside them and at the world's origin; views clamped at each edge, one behind its camera (w <= 0),
    non-finite and negative cells."""
    from deepfly3d_amd import heatmap3d

    c = hc.special(V)
    pts = hc.probe_points(c)
    got = heatmap3d.heatmap_scores(c["P"], _dev(c["hm"], cuda), c["flip"], c["plane"], _dev(pts, cuda), hc.IMAGE_SHAPE).cpu().numpy()
    want = ho.scores(c["hm"], c["P"], c["flip"], c["plane"], pts, hc.IMAGE_SHAPE, hc.FLOOR)
    print(f"special({V}): |device - oracle| {np.abs(got - want).max():.2e}, scores {want.min():.3f} .. {want.max():.3f}")
    assert np.isfinite(got).all() and np.abs(got - want).max() <= SCORE_BAR
    lf = float(np.log(hc.FLOOR))
    assert (got[:, :3, 1] == sum([lf] * V)).all() and (got[:, 3] >= lf).all()   # off every plane: the floor of every view; joint 3: one view


# ---------------------------------------------------------------------------------------------------------------------- the search
CASES = {"fly": ("fly", (2,), {}), "fly, noise 0.02": ("fly", (2, 0.02), {}), "special 2": ("special", (2,), {}), "special 3": ("special", (3,), {}),
         "special 8": ("special", (8,), {}), "one level": ("special", (8,), {"levels": 1}), "six levels": ("special", (8,), {"levels": 6}),
         "half 2.0: the planes": ("special", (3,), {"half": 2.0})}


def _compare(name, r, ref, case):
    got = {f: getattr(r, f).cpu().numpy() for f in FIELDS}
    return hc.compare(name, got, r.path.cpu().numpy(), ref, case["X0"], hc.comparable(ref), POINT_BAR, SCORE_BAR, what=f"under the gap of {hc.GAP:g}")


@pytest.mark.parametrize("name", list(CASES))
def test_search_against_the_oracle(native_lib, cuda, name):
    maker, args, kw = CASES[name]
    case, ref = getattr(hc, maker)(*args), hc.reference(maker, *args, **kw)
    r = _search(case, cuda, **kw)
    path = _compare(name, r, ref, case)
    assert r.params == (kw.get("half", hc.HALF), kw.get("levels", hc.LEVELS), hc.FLOOR, 8)
    if name in ("fly", "fly, noise 0.02", "special 3"):
        assert (path[path != 0] == 1).all()     # at the defaults three views' windows fit the budget ...
    if name.startswith("half 2.0"):
        assert (path[path != 0] == 2).all()     # ... and at five times the cube they do not
    # two runs hold the same bits
    again = _search(case, cuda, **kw)
    assert all(_same_bits(getattr(r, f), getattr(again, f)) for f in FIELDS)


@pytest.mark.parametrize("name", ["fly, noise 0.02", "special 2", "special 3", "six levels"])
def test_the_lds_route_and_the_plane_route_hold_the_same_bits(native_lib, cuda, name):
    from deepfly3d_amd import heatmap3d

    maker, args, kw = CASES[name]
    case = getattr(hc, maker)(*args)
    staged, planes = _search(case, cuda, **kw), _search(case, cuda, budget=0, **kw)
    sp, pp = staged.path.cpu().numpy(), planes.path.cpu().numpy()
    print(f"{name}: {int((sp == 1).sum())} of {int((sp != 0).sum())} searches staged their windows (budget {heatmap3d.window_doubles()} cells)")
    assert (sp == 1).any() and not (pp == 1).any() and np.array_equal(sp == 0, pp == 0)
    assert all(_same_bits(getattr(staged, f), getattr(planes, f)) for f in FIELDS)
    small = _search(case, cuda, budget=600, **kw)   # a budget between the joints' needs: some staged, some not, the same bits
    assert all(_same_bits(getattr(staged, f), getattr(small, f)) for f in FIELDS)


def test_no_frames(native_lib, cuda):
    case = hc.special(3)
    empty = dict(case, hm=case["hm"][:0], X0=case["X0"][:0])
    r = _search(empty, cuda)
    assert tuple(r.points3d.shape) == (0, 4, 3) and tuple(r.choice.shape) == (0, 4, hc.LEVELS) and not r.counts.any()


def test_bytes_past_every_output_stay_untouched(native_lib, cuda):
    from deepfly3d_amd import _native, heatmap3d

    case = hc.special(8)
    n, V, C, H, W = case["hm"].shape
    J, PAD, levels = case["plane"].shape[1], 64, 3
    hm, X0 = _dev(case["hm"], cuda), _dev(case["X0"], cuda)
    sizes = dict(X=n * J * 24, score=n * J * 8, status=n * J, views=n * J * 4, shift=n * J * 8, choice=n * J * levels * 4, counts=J * 32, path=n * J)
    bufs = {k: torch.full((v + PAD,), 0xA5, dtype=torch.uint8, device=cuda) for k, v in sizes.items()}
    dp, bp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
    P, flip, plane = np.ascontiguousarray(case["P"]), np.ascontiguousarray(case["flip"]), np.ascontiguousarray(case["plane"])
    rc = native_lib.df3d_triangulate_heatmaps(hm.data_ptr(), n, V, C, H, W, P.ctypes.data_as(dp), flip.ctypes.data_as(bp), plane.ctypes.data_as(ip), J,
                                              X0.data_ptr(), hc.HALF, levels, 7.5, 7.5, float(np.log(hc.FLOOR)), heatmap3d.window_doubles(),
                                              *(bufs[k].data_ptr() for k in sizes), torch.cuda.current_stream(cuda).cuda_stream)
    _native.check(rc, "df3d_triangulate_heatmaps")
    torch.cuda.synchronize()
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), k
    want = _search(case, cuda, levels=levels)
    for k, f in (("X", "points3d"), ("score", "score"), ("status", "status"), ("views", "views"), ("shift", "shift"), ("choice", "choice"),
                 ("counts", "counts"), ("path", "path")):
        assert torch.equal(bufs[k][:sizes[k]], getattr(want, f).contiguous().view(torch.uint8).reshape(-1)), k
    pts = _dev(hc.probe_points(case, M=5), cuda)
    out = torch.full((n * J * 5 * 8 + PAD,), 0xA5, dtype=torch.uint8, device=cuda)
    rc = native_lib.df3d_heatmap3d_scores(hm.data_ptr(), n, V, C, H, W, P.ctypes.data_as(dp), flip.ctypes.data_as(bp), plane.ctypes.data_as(ip), J,
                                          pts.data_ptr(), 5, 7.5, 7.5, float(np.log(hc.FLOOR)), out.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
    _native.check(rc, "df3d_heatmap3d_scores")
    torch.cuda.synchronize()
    assert (out[n * J * 5 * 8:] == 0xA5).all() and not (out[:n * J * 5 * 8] == 0xA5).all()


# ---- Core and the CLI on the two golden frames, synthetic weights -------------------------------------------------------------------
def _copy_images(golden_dir, folder):
    os.makedirs(folder)
    for f in os.listdir(os.path.join(golden_dir, "images")):
        shutil.copy(os.path.join(golden_dir, "images", f), folder)
    return folder


def _result_bytes(folder):
    out_dir = folder + "_df3d"
    names = [f for f in os.listdir(out_dir) if f.startswith("df3d_result")]
    assert len(names) == 1
    with open(os.path.join(out_dir, names[0]), "rb") as f:
        return f.read()


def _same_value(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same_value(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_core_and_cli_on_the_golden_frames(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    from deepfly3d_amd import cli, heatmap3d
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    config.pop("image_shape", None)
    folder = _copy_images(golden_dir, str(tmp_path / "plain" / "images"))
    assert cli.main([folder, "-n", "2"]) == 0
    baseline = _result_bytes(folder)
    plain = pickle.loads(baseline)
    # the flag: the seven keys last, every other key what the plain run wrote
    config.pop("image_shape", None)
    folder = _copy_images(golden_dir, str(tmp_path / "flag" / "images"))
    assert cli.main([folder, "-n", "2", "--heatmap-triangulation"]) == 0
    run = pickle.loads(_result_bytes(folder))
    assert list(run) == list(plain) + list(Core._HEATMAP3D_KEYS) and len(Core._HEATMAP3D_KEYS) == 7
    assert all(_same_value(run[k], plain[k]) for k in plain)
    T = plain["points2d"].shape[1]
    assert T == 2 and run["points3d_heatmap"].shape == (T, 38, 3) and run["heatmap3d_status"].shape == (T, 38) and run["heatmap3d_status"].dtype == np.int8
    assert run["heatmap3d_score"].shape == (T, 38) and run["heatmap3d_views"].dtype == np.int32 and run["heatmap3d_shift"].shape == (T, 38)
    assert run["heatmap3d_counts"].shape == (38, 4) and run["heatmap3d_counts"].sum() == T * 38
    assert run["heatmap3d_params"].tolist() == [hc.HALF, float(hc.LEVELS), hc.FLOOR, 8.0]
    keeps = np.isin(run["heatmap3d_status"], (0, 2))
    assert run["points3d_heatmap"][keeps].tobytes() == plain["points3d_wo_procrustes"][keeps].tobytes()
    print(f"golden frames, synthetic weights: statuses {run['heatmap3d_counts'].sum(axis=0).tolist()}, largest shift {run['heatmap3d_shift'].max():.3f} mm")
    # Core on the earlier result: the method, and the same search on Core.heatmaps and the save's own triangulation
    core = Core(folder, None, 2)
    core.save()
    before = _result_bytes(folder)
    assert _same_value(pickle.loads(before), {k: run[k] for k in plain})
    r = core.heatmap_triangulation()
    assert isinstance(r, heatmap3d.HeatmapTriangulation) and isinstance(r.points3d, np.ndarray)
    for key, value in zip(Core._HEATMAP3D_KEYS[:6], (r.points3d, r.status, r.score, r.views, r.shift, r.counts)):
        assert _same_value(run[key], value), key
    cameras, flip, plane = heatmap3d.view_table(core.camera_ordering)
    hm = torch.stack([core.heatmaps(i)[torch.from_numpy(cameras).to(cuda)] for i in range(T)]).contiguous()
    P = np.stack([c.P for c in core.camNet.cam_list])[cameras]
    want = heatmap3d.triangulate_heatmaps(P, hm, flip, plane, _dev(plain["points3d_wo_procrustes"], cuda), core.image_shape)
    assert _same_value(want.points3d.cpu().numpy(), r.points3d) and _same_value(want.choice.cpu().numpy(), r.choice)
    assert _same_value(want.score.cpu().numpy(), r.score)
    # parameters, with --skip-pose-estimation while the images are present
    assert cli.main([folder, "-n", "2", "--skip-pose-estimation", "--heatmap-triangulation", "--heatmap-levels", "2", "--heatmap-half", "0.2"]) == 0
    again = pickle.loads(_result_bytes(folder))
    assert list(again) == list(run) and again["heatmap3d_params"].tolist() == [0.2, 2.0, hc.FLOOR, 8.0]
    # the stages: robust -> heat-map -> repair, the angles from the repaired heat-map pose
    core.save(joint_angles=True, repair_pose=True, robust_triangulation=True, heatmap_triangulation=True)
    staged = pickle.loads(_result_bytes(folder))
    assert list(staged) == (list(plain) + ["joint_angles", "segment_lengths"] + list(Core._REPAIR_KEYS) + list(Core._ROBUST_KEYS)
                            + list(Core._HEATMAP3D_KEYS))
    from deepfly3d_amd import ops

    want = heatmap3d.triangulate_heatmaps(P, hm, flip, plane, _dev(staged["points3d_robust"], cuda), core.image_shape)
    assert _same_value(staged["points3d_heatmap"], want.points3d.cpu().numpy())
    assert _same_value(staged["points3d_repaired"], ops.repair_pose(want.points3d).points.cpu().numpy())
    with pytest.raises(ValueError, match="heatmap_half, heatmap_levels and heatmap_floor belong to heatmap_triangulation"):
        core.save(heatmap_levels=3)
    # without the flag the file is what it was before the flag, byte for byte
    assert _result_bytes(folder) != before
    core.save()
    assert _result_bytes(folder) == before
    # without the images there is nothing to search
    for f in os.listdir(folder):
        os.remove(os.path.join(folder, f))
    with pytest.raises(FileNotFoundError, match="holds none"):
        core.heatmap_triangulation()
    config.pop("image_shape", None)
