"""-m gpu sweep of the heat-map triangulation (csrc/heatmap3d.hip, DESIGN.md section 25, "swept") over the families of
tests/heatmap3d_cases.py, which tests/test_heatmap3d_cases_host.py certifies on the CPU: plane shapes from 4 x 4 to 1 024 x 1 024 with
unequal cells, the widest tables, exact ties, windows that fill the LDS array to its last double and pass it by one row, a camera plane
that cuts the reachable cube, a floor that is a float32, 70 400 workgroups, and Core's batches.  Everything discrete is compared exactly
wherever the oracle's search is firm at every level (heatmap3d_cases.firm), the rest within the bars of tests/test_gpu_heatmap3d.py,
re-derived by that file's formulas for each case's magnitudes (heatmap3d_cases.point_bar, score_bar)."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import heatmap3d_cases as hc
import heatmap3d_oracle as ho

pytestmark = pytest.mark.gpu

FIELDS = hc.FIELDS
SEARCHES = [name for family, names in hc.FAMILIES.items() if family != "many" for name in names]


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the cached cases are read-only


def _search(c, cuda, **kw):
    from deepfly3d_amd import heatmap3d

    return heatmap3d.triangulate_heatmaps(c["P"], _dev(c["hm"], cuda), c["flip"], c["plane"], _dev(c["X0"], cuda), c["image_shape"], half=c["half"],
                                          levels=c["levels"], floor=c["floor"], **kw)


def _host(r):
    return {f: getattr(r, f).cpu().numpy() for f in FIELDS}


def _same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in ((a[f], b[f]) for f in FIELDS))


def _firm_compare(name, r, cuda):
    c, ref = hc.sweep(name), hc.sweep_reference(name)
    ok = hc.firm(c, ref)
    got, path = _host(r), r.path.cpu().numpy()
    hc.compare(name, got, path, ref, c["X0"], ok, hc.point_bar(c), hc.score_bar(c), what="not firm")
    moved = ok & (ref["status"] % 2 == 1)
    print(f"{name}: smallest gap_next {ref['gap_next'].min():.2e}, {int((ref['ties'] >= 2).sum())} tied levels, |points| "
          f"{np.abs(got['points3d'][moved] - ref['points'][moved]).max(initial=0.0):.2e} (bar {hc.point_bar(c):.1e}), score bar {hc.score_bar(c):.1e}")
    return got, path, ref, ok


# ------------------------------------------------------------------------------------------------------------------- every family
@pytest.mark.parametrize("name", [n for n in SEARCHES if n != "ties"])
def test_the_sampler_on_every_shape(native_lib, cuda, name):
    """heatmap_scores on the plane's four edges exactly, just outside them, inside and at random (probe_points for the golden cameras)."""
    from deepfly3d_amd import heatmap3d

    c, pts = hc.sweep(name), hc.sweep_points(name)
    got = heatmap3d.heatmap_scores(c["P"], _dev(c["hm"], cuda), c["flip"], c["plane"], _dev(pts, cuda), c["image_shape"], floor=c["floor"]).cpu().numpy()
    with np.errstate(all="ignore"):
        want = ho.scores(c["hm"], c["P"], c["flip"], c["plane"], pts, c["image_shape"], c["floor"])
    lf = float(np.log(c["floor"]))
    base = np.array([sum([lf] * int((c["plane"][:, j] >= 0).sum()), 0.0) for j in range(c["plane"].shape[1])])[None, :, None]
    print(f"{name}: |device - oracle| {np.abs(got - want).max():.2e} over {want.size} points, {int((want == base).sum())} of them at the floor of every "
          f"view, scores {want.min():.3f} .. {want.max():.3f}")
    assert got.shape == want.shape and np.isfinite(got).all() and np.abs(got - want).max() <= hc.score_bar(c)
    assert np.array_equal(got == base, want == base)       # "no evidence" is the floor itself on both sides, to the bit


@pytest.mark.parametrize("name", SEARCHES)
def test_search_against_the_oracle(native_lib, cuda, name):
    r = _search(hc.sweep(name), cuda)
    got, path, ref, ok = _firm_compare(name, r, cuda)
    if name in hc.NONE_LEFT_OUT:
        assert ok.all()
    assert _same_bits(got, _host(_search(hc.sweep(name), cuda)))   # two runs hold the same bits


def test_ties_go_to_the_lowest_index(native_lib, cuda):
    """A lane's own pair, the lower index in the higher lane, a pair four steps apart, and eight equal points in eight neighbouring lanes:
    the choice is the oracle's first of equals at every level, and the next level's centre follows it."""
    for name in ("ties", "budget behind"):
        c, ref = hc.sweep(name), hc.sweep_reference(name)
        got = _host(_search(c, cuda))
        assert (ref["ties"][:, :, 0] >= 2).all() and hc.firm(c, ref).all()
        assert np.array_equal(got["choice"], ref["choice"]) and np.array_equal(got["status"], ref["status"])
        assert np.abs(got["points3d"] - ref["points"]).max() <= hc.point_bar(c) and np.abs(got["score"] - ref["score"]).max() <= hc.score_bar(c)
    assert hc.sweep_reference("ties")["choice"][0, :, 0].tolist() == [a for a, _ in hc.TIE_PAIRS]
    # a single level: nothing after the tie can repair or hide the choice
    c = dict(hc.sweep("ties"), levels=1)
    one = _host(_search(c, cuda))
    pts = np.array([hc.level_points(c, hc.sweep_reference("ties"), 0, k, 0)[0][a] for k, (a, _) in enumerate(hc.TIE_PAIRS)])
    assert one["choice"][0, :, 0].tolist() == [a for a, _ in hc.TIE_PAIRS] and np.abs(one["points3d"][0] - pts).max() <= hc.point_bar(c)


# ---------------------------------------------------------------------------------------------------------------------- the route
def _budgets(used):
    """Budgets on both sides of the smallest, the middle and the largest need of the case's searches, and the ends."""
    u = np.unique(used[used > 0])
    picks = sorted({int(u[0]), int(u[len(u) // 2]), int(u[-1])})
    return sorted({b for x in picks for b in (x, x - 1) if 0 <= b <= 4096} | {0, 4096})


@pytest.mark.parametrize("name", hc.ROUTES)
def test_the_route_follows_the_window_model(native_lib, cuda, name):
    """path == 1 exactly where the model's windows hold 0 < used <= budget cells, for budgets at a search's own need and one under it;
    the results do not know the route."""
    from deepfly3d_amd import heatmap3d

    assert heatmap3d.window_doubles() == 4096
    c, used = hc.sweep(name), hc.sweep_windows(name)[0]
    searched = hc.sweep_reference(name)["status"] != 0
    budgets = _budgets(used)
    first, seen = None, set()
    for b in budgets:
        r = _search(c, cuda, budget=b)
        got, path = _host(r), r.path.cpu().numpy()
        want = np.where(searched, np.where((used > 0) & (used <= b), 1, 2), 0)
        assert np.array_equal(path, want), (name, b, path.tolist(), used.tolist())
        first = got if first is None else first
        assert _same_bits(first, got), (name, b)
        seen |= set(path.ravel().tolist())
    print(f"{name}: used {int(used[used > 0].min())} .. {int(used.max())} cells, budgets {budgets}, routes seen {sorted(seen)}")
    assert {1, 2} <= seen or (used.min() > 4096 and seen == {2})   # a case that passes the array at every budget has one route
    default = _search(c, cuda).path.cpu().numpy()
    assert np.array_equal(default, np.where(searched, np.where(used <= 4096, 1, 2), 0))
    if name == "special 8":   # the one search whose eight windows pass the budget, beside staged neighbours
        assert np.argwhere(default == 2).tolist() == [[2, 2]] and (default == 1).sum() == 6


def test_a_window_that_fills_the_lds_array(native_lib, cuda):
    """used == 4096: staged, the last double of the array written and read, the bits of the plane route, nothing past any output."""
    from deepfly3d_amd import _native, heatmap3d

    c = hc.sweep("budget 4096")
    assert (hc.sweep_windows("budget 4096")[0] == heatmap3d.window_doubles()).all()
    n, V, C, H, W = c["hm"].shape
    J, PAD, levels = c["plane"].shape[1], 64, c["levels"]
    hm, X0 = _dev(c["hm"], cuda), _dev(c["X0"], cuda)
    sizes = dict(X=n * J * 24, score=n * J * 8, status=n * J, views=n * J * 4, shift=n * J * 8, choice=n * J * levels * 4, counts=J * 32, path=n * J)
    bufs = {k: torch.full((v + PAD,), 0xA5, dtype=torch.uint8, device=cuda) for k, v in sizes.items()}
    dp, bp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
    P, flip, plane = np.ascontiguousarray(c["P"]), np.ascontiguousarray(c["flip"]), np.ascontiguousarray(c["plane"])
    rc = native_lib.df3d_triangulate_heatmaps(hm.data_ptr(), n, V, C, H, W, P.ctypes.data_as(dp), flip.ctypes.data_as(bp), plane.ctypes.data_as(ip), J,
                                              X0.data_ptr(), c["half"], levels, 4.0, 8.0, float(np.log(c["floor"])), heatmap3d.window_doubles(),
                                              *(bufs[k].data_ptr() for k in sizes), torch.cuda.current_stream(cuda).cuda_stream)
    _native.check(rc, "df3d_triangulate_heatmaps")
    torch.cuda.synchronize()
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), k
    assert (bufs["path"][:n * J] == 1).all()
    staged, planes = _search(c, cuda), _search(c, cuda, budget=0)
    assert (staged.path == 1).all() and (planes.path == 2).all() and _same_bits(_host(staged), _host(planes))
    for k, f in (("X", "points3d"), ("score", "score"), ("status", "status"), ("views", "views"), ("shift", "shift"), ("choice", "choice"),
                 ("counts", "counts"), ("path", "path")):
        assert torch.equal(bufs[k][:sizes[k]], getattr(staged, f).contiguous().view(torch.uint8).reshape(-1)), k
    _firm_compare("budget 4096", staged, cuda)


# ------------------------------------------------------------------------------------------------------------------- many frames
def test_more_workgroups_than_65535(native_lib, cuda):
    """n = 1 100 frames of 64 joints, 70 400 workgroups: every frame is a copy of one of four, and holds that frame's bytes."""
    c, ref = hc.sweep("many"), hc.sweep_reference("many")
    four = _search(c, cuda)
    got4, path4, ref, ok = _firm_compare("many", four, cuda)
    R = hc.MANY_REPEAT
    big = dict(c, hm=np.tile(c["hm"], (R, 1, 1, 1, 1)), X0=np.tile(c["X0"], (R, 1, 1)))
    assert big["hm"].shape[0] * c["plane"].shape[1] == 70400
    r = _search(big, cuda)
    got = _host(r)
    for f in FIELDS[:-1]:
        assert got[f].tobytes() == np.tile(got4[f], (R,) + (1,) * (got4[f].ndim - 1)).tobytes(), f
    assert r.path.cpu().numpy().tobytes() == np.tile(path4, (R, 1)).tobytes()
    assert np.array_equal(got["counts"], ref["counts"] * R) and np.array_equal(got["counts"], got4["counts"] * R) and got["counts"].sum() == 70400


# --------------------------------------------------------------------------------------------------------------------------- Core
def test_core_batches_of_one_and_of_sixteen(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    """Core._heatmap3d_on runs the frames in batches, concatenates eight fields and sums the counts: the two golden frames one by one
    and in one batch hold the same bits."""
    from deepfly3d_amd import cli, heatmap3d
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    config.pop("image_shape", None)
    folder = str(tmp_path / "images")
    os.makedirs(folder)
    for f in os.listdir(os.path.join(golden_dir, "images")):
        shutil.copy(os.path.join(golden_dir, "images", f), folder)
    assert cli.main([folder, "-n", "2"]) == 0
    core = Core(folder, None, 2)
    params = heatmap3d.heatmap3d_params()
    one = core._heatmap3d_on("heatmap_triangulation", params, batch=1)
    both = core._heatmap3d_on("heatmap_triangulation", params)
    a, b = _host(one), _host(both)
    assert a["points3d"].shape == (2, 38, 3) and a["counts"].shape == (38, 4) and one.params == both.params
    for f in FIELDS:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes(), f
    assert one.path.cpu().numpy().tobytes() == both.path.cpu().numpy().tobytes()
    assert a["counts"].sum() == 2 * 38 and np.array_equal(a["counts"], np.stack([(a["status"] == k).sum(axis=0) for k in range(4)], axis=1))
    print(f"golden frames, batches of 1 and of 16: statuses {a['counts'].sum(axis=0).tolist()}")
    config.pop("image_shape", None)
