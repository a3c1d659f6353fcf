"""-m gpu tests of the opt-in sub-pixel localisation of heat-map peaks: df3d_heatmap_argmax_subpixel and
df3d_heatmap_peaks_subpixel against the float64 numpy statement of the rule (tests/subpixel_oracle.py) BIT FOR BIT, the plain entries
unchanged beside them, the option through inference_folder and Core, and what it buys in 3-D on the golden rig."""
import os
import pickle

import numpy as np
import pytest
import torch

import subpixel_oracle as so
from oracle import geometry as og

pytestmark = pytest.mark.gpu

H, W = 64, 128


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _both(hm, cuda):
    """(plain points, plain conf, refined points, refined conf, non-finite counts of the two calls) of hm [n, J, h, w] float32 numpy."""
    from deepfly3d_amd import ops

    d = torch.from_numpy(np.ascontiguousarray(hm, np.float32)).to(cuda)
    f0 = torch.zeros(1, dtype=torch.int32, device=cuda)
    f1 = torch.zeros(1, dtype=torch.int32, device=cuda)
    p0, c0 = ops.heatmap_argmax(d, nonfinite=f0)
    p1, c1 = ops.heatmap_argmax(d, nonfinite=f1, subpixel=True)
    return p0.cpu().numpy(), c0.cpu().numpy(), p1.cpu().numpy(), c1.cpu().numpy(), int(f0.item()), int(f1.item())


def _check_argmax(hm, cuda, plain_oracle=True):
    hm = np.ascontiguousarray(hm, np.float32)
    p0, c0, p1, c1, f0, f1 = _both(hm, cuda)
    want_p, want_c = so.heatmap_argmax_subpixel(hm)
    bad = np.argwhere(_bits(p1) != _bits(want_p))
    assert bad.size == 0, f"{len(bad)} coordinates differ from the oracle, first {bad[0]}: {p1[tuple(bad[0])]!r} != {want_p[tuple(bad[0])]!r}"
    assert np.array_equal(_bits(c1), _bits(want_c))
    # confidence and the non-finite counter are the plain call's; the refined point stays within half a cell of the plain one
    assert np.array_equal(_bits(c1), _bits(c0)) and f0 == f1
    assert f0 == int((~np.isfinite(hm)).any(axis=(2, 3)).sum())
    h, w = hm.shape[2:]
    assert np.all(np.abs(p1.astype(np.float64) - p0.astype(np.float64)) <= np.array([0.5 / h, 0.5 / w]))
    if plain_oracle:   # the plain call is what it was: oracle/geometry.py bit for bit (finite planes: numpy's arg-max lets a NaN win)
        rp, rc = og.heatmap_argmax(hm)
        assert np.array_equal(_bits(p0), _bits(rp)) and np.array_equal(_bits(c0), _bits(rc))
    return p0, p1


def _blobs(rng, n, J, sigmas=(1.0, 1.5, 2.0), margin=0.0):
    hm = np.zeros((n, J, H, W), np.float32)
    for a in range(n):
        for b in range(J):
            s = sigmas[(a * J + b) % len(sigmas)]
            amp = np.float32(rng.uniform(0.2, 3.0))
            hm[a, b] = amp * so.gaussian_plane(rng.uniform(margin, H - 1 - margin), rng.uniform(margin, W - 1 - margin), s, (H, W))
    return hm


@pytest.mark.parametrize("n,joints,h,w", [(4, 19, 64, 128), (3, 5, 64, 128), (13, 19, 64, 128), (3, 5, 8, 16), (2, 3, 128, 256)])
def test_subpixel_argmax_equals_the_oracle_on_random_planes(native_lib, cuda, n, joints, h, w):
    """n * J both a multiple of 4 (a full block of four waves) and not."""
    rng = np.random.default_rng(n * 1000 + h)
    p0, p1 = _check_argmax(rng.normal(size=(n, joints, h, w)).astype(np.float32), cuda)
    assert (p0 != p1).any()


@pytest.mark.parametrize("n,joints", [(4, 19), (13, 19), (1, 3)])
def test_subpixel_argmax_equals_the_oracle_on_gaussian_blobs(native_lib, cuda, n, joints):
    rng = np.random.default_rng(7 + n)
    hm = _blobs(rng, n, joints)
    p0, p1 = _check_argmax(hm, cuda)
    assert (p0 != p1).mean() > 0.5
    noisy = (hm + rng.normal(0.0, 0.02, size=hm.shape)).astype(np.float32)
    _check_argmax(noisy, cuda)


def test_subpixel_argmax_on_borders_corners_and_ties(native_lib, cuda):
    rng = np.random.default_rng(11)
    cells = [(0, 40), (H - 1, 40), (20, 0), (20, W - 1), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),   # borders and corners: no offset
             (1, 1), (H - 2, W - 2), (1, 64), (31, 126)]                                                  # one cell inside: refined
    hm = (0.1 * rng.random((len(cells), 2, H, W))).astype(np.float32)
    for a, (r, c) in enumerate(cells):
        hm[a, :, r, c] = 1.0
        if 0 < r < H - 1 and 0 < c < W - 1:
            hm[a, 1, r, c + 1] = 0.7
            hm[a, 1, r - 1, c] = 0.6
    p0, p1 = _check_argmax(hm, cuda)
    assert np.array_equal(p0[:8], p1[:8]) and (p0[8:, 1] != p1[8:, 1]).any(axis=-1).all()
    for a, (r, c) in enumerate(cells):
        assert p0[a, 0].tolist() == [r / H, c / W]
    # a Gaussian whose centre lies outside the plane or in its outermost cells: the maximum is a border cell
    edge = np.stack([so.gaussian_plane(-0.3, 50.2, 1.5), so.gaussian_plane(63.4, 50.2, 1.5), so.gaussian_plane(30.3, 0.2, 1.5),
                     so.gaussian_plane(30.3, 127.4, 1.5)])[:, None]
    p0, p1 = _check_argmax(edge, cuda)
    assert np.array_equal(p0, p1)
    # ties: two equal maxima far apart (the first wins), next to each other in a row, in a column, on a diagonal, a 2 x 2 plateau
    t = (0.1 * rng.random((6, 1, H, W))).astype(np.float32)
    t[0, 0, 10, 5] = t[0, 0, 40, 100] = 2.0
    t[1, 0, 31, 77] = t[1, 0, 31, 78] = 3.0
    t[2, 0, 31, 77] = t[2, 0, 32, 77] = 3.0
    t[3, 0, 31, 77] = t[3, 0, 32, 78] = 3.0
    t[4, 0, 31:33, 77:79] = 3.0
    t[5, 0, 20:23, 60:63] = 1.5   # a 3 x 3 plateau: its first cell wins, flat towards the plateau
    p0, p1 = _check_argmax(t, cuda)
    assert p0[0, 0].tolist() == [10 / H, 5 / W] and p0[4, 0].tolist() == [31 / H, 77 / W] and p0[5, 0].tolist() == [20 / H, 60 / W]
    assert p1[1, 0, 1] > p0[1, 0, 1] and p1[2, 0, 0] > p0[2, 0, 0]   # towards the equal neighbour
    # an all-equal plane (cell 0), all-zero planes, a plane of -inf
    flat = np.zeros((5, 1, H, W), np.float32)
    flat[1] = 0.25
    flat[2] = -3.0
    flat[3] = -np.inf
    p0, p1 = _check_argmax(flat, cuda)
    assert not p1.any()


def test_subpixel_argmax_with_non_finite_values(native_lib, cuda):
    """+inf / -inf / NaN at and beside the maximum: a non-finite value among the nine keeps the cell; a NaN never wins the arg-max."""
    rng = np.random.default_rng(13)
    base = _blobs(rng, 1, 1, sigmas=(1.5,), margin=8.0)[0, 0]
    r, c = np.unravel_index(int(base.argmax()), base.shape)
    planes = []
    for bad in (np.inf, -np.inf, np.nan):
        for dr, dc in [(0, 0), (0, 1), (-1, 0), (1, -1), (-1, -1), (0, 2), (3, 3)]:   # the last two lie outside the 3 x 3: refined as usual
            p = base.copy()
            p[r + dr, c + dc] = bad
            planes.append(p)
    planes.append(np.full((H, W), np.nan, np.float32))   # nothing can win: cell 0, the confidence is the first value
    p = base.copy()
    p[5, 5] = np.inf
    p[40, 90] = np.inf   # two infinities: the first is the arg-max
    planes.append(p)
    hm = np.stack(planes)[:, None]
    p0, p1 = _check_argmax(hm, cuda, plain_oracle=False)
    k = 7
    for b in range(3):
        assert np.array_equal(p0[b * k : b * k + 5], p1[b * k : b * k + 5])   # at or beside the maximum (+inf: it IS the maximum): the cell is kept
    for b in (1, 2):
        assert (p0[b * k + 5 : b * k + 7] != p1[b * k + 5 : b * k + 7]).any(axis=-1).all()   # -inf / NaN outside the neighbourhood: refined
    assert np.array_equal(p0[0], p1[0]) and p0[0, 0].tolist() == [r / H, c / W]               # +inf at the maximum wins and keeps its cell


@pytest.mark.parametrize("k", [1, 5, 16])
def test_subpixel_peaks_refine_the_plain_calls_cells(native_lib, cuda, k):
    from deepfly3d_amd import ops

    rng = np.random.default_rng(17 + k)
    multi = np.zeros((3, 4, H, W), np.float32)
    for a in range(3):
        for b in range(4):
            for _ in range(int(rng.integers(1, 7))):
                multi[a, b] += np.float32(rng.uniform(0.2, 1.0)) * so.gaussian_plane(rng.uniform(0, H - 1), rng.uniform(0, W - 1), rng.uniform(0.8, 2.5))
    multi[2, 3, 20, 30] = np.nan
    multi[2, 2, 11, 100] = np.inf
    multi[1, 0] = 0.5   # a flat plane: cell 0 is its only peak
    for hm in (rng.normal(size=(2, 19, H, W)).astype(np.float32), multi, rng.integers(0, 6, size=(3, 5, 8, 16)).astype(np.float32)):
        d = torch.from_numpy(hm).to(cuda)
        c0, p0, v0 = (x.cpu().numpy() for x in ops.heatmap_peaks(d, k))
        c1, p1, v1 = (x.cpu().numpy() for x in ops.heatmap_peaks(d, k, subpixel=True))
        assert np.array_equal(c0, c1) and np.array_equal(_bits(v0), _bits(v1))
        want = so.refine_peaks(hm, c0, p0)
        bad = np.argwhere(_bits(p1) != _bits(want))
        assert bad.size == 0, f"{len(bad)} peak coordinates differ from the oracle, first {bad[0]}"
        h, w = hm.shape[2:]
        assert np.all(np.abs(p1.astype(np.float64) - p0.astype(np.float64)) <= np.array([0.5 / h, 0.5 / w]))
        # peak 0 is the refined arg-max point wherever the plain peak 0 is the plain arg-max cell (the plane's maximum is finite)
        a0, _ = ops.heatmap_argmax(d)
        a1, _ = ops.heatmap_argmax(d, subpixel=True)
        a0, a1 = a0.cpu().numpy(), a1.cpu().numpy()
        same = (c0 >= 1) & (p0[:, :, 0] == a0).all(axis=-1)
        assert same.sum() >= same.size - 2
        assert np.array_equal(_bits(p1[:, :, 0][same]), _bits(a1[same]))


def _sample_folder(tmp_path, golden_dir):
    src = os.path.join(golden_dir, "images")
    folder = tmp_path / "working"
    folder.mkdir()
    for f in os.listdir(src):
        os.symlink(os.path.join(src, f), folder / f)
    return str(folder)


def test_subpixel_through_the_network(native_lib, cuda, tmp_path, golden_dir):
    """inference_folder(subpixel=True) on the sample images with synthetic weights: the points are the oracle's on the returned heat-maps,
    within half a cell of the plain run's; the confidences are the plain run's; the peaks are refined too."""
    from deepfly3d_amd import inference
    from deepfly3d_amd.synthetic import synthetic_state_dict

    sd = synthetic_state_dict(0)
    folder = _sample_folder(tmp_path, golden_dir)
    kw = dict(folder=folder, camera_ids_to_flip=[4, 5, 6], return_heatmap=True, return_confidence=True, max_img_id=1, batch_size=8, state_dict=sd)
    p0, hm0, c0 = inference.inference_folder(**kw)
    p1, hm1, c1 = inference.inference_folder(subpixel=True, **kw)
    assert p1.shape == p0.shape == (7, 2, 19, 2) and p1.dtype == np.float32 and c1.shape == (7, 2, 19, 1)
    assert np.array_equal(hm0, hm1) and np.array_equal(_bits(c0), _bits(c1))
    want_p, want_c = so.heatmap_argmax_subpixel(hm1.reshape(14, 19, H, W))
    assert np.array_equal(_bits(p1.reshape(14, 19, 2)), _bits(want_p)) and np.array_equal(_bits(c1.reshape(14, 19)), _bits(want_c))
    assert np.all(np.abs(p1.astype(np.float64) - p0.astype(np.float64)) <= np.array([0.5 / H, 0.5 / W]))
    assert (p1 != p0).any()
    out = inference.inference_folder(subpixel=True, return_peaks=4, **kw)
    assert len(out) == 6 and np.array_equal(_bits(out[0]), _bits(p1))
    cnt, pp, pv = out[3:]
    plain = inference.inference_folder(return_peaks=4, **kw)
    assert np.array_equal(cnt, plain[3]) and np.array_equal(_bits(pv), _bits(plain[5])) and pp.shape == (7, 2, 19, 4, 2)
    want = so.refine_peaks(hm1.reshape(14, 19, H, W), plain[3].reshape(14, 19), plain[4].reshape(14, 19, 4, 2))
    assert np.array_equal(_bits(pp.reshape(14, 19, 4, 2)), _bits(want))


# ------------------------------------------------------------------------------------------------ 3-D on the golden rig
IMG_H, IMG_W = 480.0, 960.0
SIGMA = 1.5


def golden_scene(golden_dir):
    """The golden rig as ground truth: P [7, 3, 4], X [15, 38, 3], seen [7, 15, 38] (the fixture's own visibility), and the true position of
    every seen joint in heat-map cells, cells [7, 15, 38, 2] (row, col)."""
    g = np.load(f"{golden_dir}/golden_3d.npz")
    P = og.projection_matrices(g["R"], g["tvec"], g["intr"])
    X = g["points3d_wo_procrustes"]
    seen = (g["points2d"] != 0).all(axis=-1)
    seen &= (seen.sum(axis=0) >= 2)[None]
    Xh = np.concatenate([X, np.ones(X.shape[:2] + (1,))], axis=-1)
    u = np.einsum("cij,tkj->ctki", P, Xh)
    col_px, row_px = u[..., 0] / u[..., 2], u[..., 1] / u[..., 2]
    cells = np.stack([row_px / IMG_H * H, col_px / IMG_W * W], axis=-1)
    return P, X, seen, cells, [int(c) for c in g["camera_ordering"]]


def counted_joints(seen, cells):
    """[15, 38] bool: seen by >= 2 cameras and at least two cells from every border in every seeing camera."""
    inside = (cells[..., 0] >= 2) & (cells[..., 0] <= H - 1 - 2) & (cells[..., 1] >= 2) & (cells[..., 1] <= W - 1 - 2)
    return seen.any(axis=0) & (inside | ~seen).all(axis=0)


def test_subpixel_recovers_the_golden_rig_in_3d(native_lib, cuda, golden_dir):
    """No network: every seen joint of tests/golden/golden_3d.npz projected into its cameras, rendered as a float32 Gaussian heat-map
    (sigma 1.5 cells), localised on the GPU (plain and refined) and triangulated with ops.triangulate.  With the rule in numpy and a
    float64 SVD DLT: 569 of 570 joints count, mean 3-D error 7.49e-3 mm with the arg-max and 4.34e-4 mm refined (maxima 4.2e-2 / 1.9e-3);
    the bounds leave 7 % and 15 %.  Then the same scene through the 19 -> 38 re-layout with the maps of the flipped cameras mirrored: the
    un-flip mirrors the offset with the cell."""
    from deepfly3d_amd import ops

    P, X, seen, cells, ordering = golden_scene(golden_dir)
    count = counted_joints(seen, cells)
    nseen = int(seen.any(axis=0).sum())
    print(f"{int(count.sum())} of {nseen} seen joints count")
    assert count.sum() >= 0.95 * nseen

    idx = np.argwhere(seen)   # (camera, frame, joint) of every rendered plane
    hm = np.stack([so.gaussian_plane(*cells[c, t, j], SIGMA, (H, W)) for c, t, j in idx])[:, None]
    d = torch.from_numpy(hm).to(cuda)
    scale = np.array([IMG_H, IMG_W])
    X3 = {}
    for name, sub in (("plain", False), ("refined", True)):
        pts, _ = ops.heatmap_argmax(d, subpixel=sub)
        px = np.zeros((7, 15, 38, 2))
        px[tuple(idx.T)] = pts.cpu().numpy()[:, 0].astype(np.float64) * scale
        X3[name] = ops.triangulate(P, torch.from_numpy(px).to(cuda)).cpu().numpy()
    err = {k: np.linalg.norm(v - X, axis=-1)[count] for k, v in X3.items()}
    for k, e in err.items():
        print(f"{k}: mean 3-D error {e.mean():.4e} mm, max {e.max():.4e} mm")
    print(f"ratio of the means {err['plain'].mean() / err['refined'].mean():.2f}")
    assert err["refined"].mean() <= 5e-4
    assert err["plain"].mean() >= 7e-3

    # through relayout_19_to_38: the network's 19 planes per view, the maps of the flipped cameras (positions 4..6 of the ordering)
    # rendered at col -> 128 - col, which the re-layout's col -> 1 - col undoes
    flipped = set(ordering[4:])
    hm19 = np.zeros((7, 15, 19, H, W), np.float32)
    for c, t, j in idx:
        r_, c_ = cells[c, t, j]
        hm19[c, t, j % 19] = so.gaussian_plane(r_, W - c_ if c in flipped else c_, SIGMA, (H, W))
    pts19, _ = ops.heatmap_argmax(torch.from_numpy(hm19.reshape(7 * 15, 19, H, W)).to(cuda), subpixel=True)
    p38 = ops.relayout_19_to_38(pts19.reshape(7, 15, 19, 2).contiguous(), ordering)
    vis = (p38.cpu().numpy() != 0).all(axis=-1)
    assert np.array_equal(vis & count[None], seen & count[None])
    Xr = ops.triangulate(P, (p38 * torch.tensor(scale, device=cuda)).contiguous()).cpu().numpy()
    diff = np.linalg.norm(Xr - X3["refined"], axis=-1)[count]
    print(f"re-layout construction against the direct one: max {diff.max():.3e} mm")
    assert diff.max() <= 1e-5


# ------------------------------------------------------------------------------------------------ Core
REFERENCE_KEYS = ["0", "1", "2", "3", "4", "5", "6", "points3d", "points2d", "points3d_wo_procrustes", "camera_ordering", "heatmap_confidence"]


@pytest.mark.parametrize("subpixel", [True, False])
def test_core_saves_the_subpixel_key_after_the_reference_keys(native_lib, cuda, tmp_path, golden_dir, monkeypatch, subpixel):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    folder = _sample_folder(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=2, camera_ordering=[0, 1, 2, 3, 4, 5, 6])
    if subpixel:
        core.pose2d_estimation(batch_size=7, subpixel=True)
    else:
        core.pose2d_estimation(batch_size=7)
    core.calibrate_calc(0, core.max_img_id)
    core.save()
    with open(core.save_path, "rb") as f:
        d = pickle.load(f)
    assert [str(k) for k in d.keys()] == REFERENCE_KEYS + (["subpixel"] if subpixel else [])
    grid = d["points2d"] * np.array([float(H), float(W)])
    if subpixel:
        assert d["subpixel"] is True and not np.array_equal(grid, np.round(grid))
    else:
        assert np.array_equal(grid, np.round(grid))
    assert d["points2d"].shape == (7, 2, 38, 2) and d["heatmap_confidence"].shape == (7, 2, 19, 1)
    config.pop("image_shape", None)
