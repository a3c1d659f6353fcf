"""GPU tests of the suspect-detection search: df3d_reproj_errors against the float64 oracle
tests/reproj_oracle.py on the golden recording, on triangulate_bits.npz and on a seeded sweep with poisoned outputs;
ops.reprojection_errors(frames=); planted outliers; Core's error navigation end to end; auto_correct(flagged_only=True) and
df3d-cli --auto-correct --correct-only-flagged on one and two ranks."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import reproj_oracle as ro

pytestmark = pytest.mark.gpu

ORDER = [0, 1, 2, 3, 4, 5, 6]
HW = np.array([480.0, 960.0])   # (H, W): normalised -> pixels
ATOL, RTOL, NEAR = 1e-9, 1e-12, 1e-9


def _cams(golden_dir):
    from oracle import geometry as og

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    return og.projection_matrices(g3["R"], g3["tvec"], g3["intr"]), g3


def _compare(got, want, thr):
    """err / jmax within ATOL or RTOL (infinities equal), masks identical apart from joints within NEAR of their threshold."""
    (ge, gj, gm), (we, wj, wm) = [tuple(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a) for a in x) for x in (got, want)]
    for g, w in ((ge, we), (gj, wj)):
        assert g.shape == w.shape and not np.isnan(g).any()
        inf = np.isinf(w)
        assert np.array_equal(np.isinf(g), inf)
        d = np.abs(g[~inf] - w[~inf])
        assert np.all((d <= ATOL) | (d <= RTOL * np.abs(w[~inf]))), d.max()
    J = wj.shape[1]
    with np.errstate(invalid="ignore"):   # inf - inf: an infinite error at a disabled joint is not near its threshold
        near = np.abs(wj - np.asarray(thr)[None, :]) <= NEAR
    fg, fw = ro.flags(gm, J), ro.flags(wm, J)
    assert np.array_equal(fg[~near], fw[~near])
    assert np.array_equal(gm[~near.any(1)], wm[~near.any(1)])


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(cuda) for a in arrays]


# ------------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("thr", [40.0, 5.0, 2.0])
def test_golden_recording_matches_the_oracle(native_lib, cuda, golden_dir, thr):
    from deepfly3d_amd import ops

    P, g3 = _cams(golden_dir)
    (px,) = _dev(cuda, g3["points2d"] * HW)
    t = np.full(38, thr)
    t[::5] = np.inf
    err, jmax, mask = ops.reprojection_errors(P, px, thresholds=t)
    X = ops.triangulate(P, px)
    want = ro.reproj_errors(P, px.cpu().numpy(), X.cpu().numpy(), t)
    _compare((err, jmax, mask), want, t)
    if thr < 40:
        assert 0 < ro.flags(want[2], 38).sum() < 15 * 38


def test_triangulate_bits_fixture_matches_the_oracle(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops

    b = np.load(f"{golden_dir}/triangulate_bits.npz")
    px, X = _dev(cuda, b["random_px"], b["random_X"])
    rng = np.random.default_rng(7)
    for thr in (np.full(38, 40.0), rng.uniform(0, 30, 38)):
        got = ops.reprojection_errors(b["P"], px, X=X, thresholds=thr)
        _compare(got, ro.reproj_errors(b["P"], b["random_px"], b["random_X"], thr), thr)


# ------------------------------------------------------------------------------------------------------------------ sweep
def _random_problem(rng, ncam, T, J):
    """Cameras on a ring looking at the origin, points near it, 0..3 (or more) views per joint, some points behind a camera."""
    P = np.zeros((ncam, 3, 4))
    centres = np.zeros((ncam, 3))
    for c in range(ncam):
        a = 2 * np.pi * c / ncam + rng.uniform(-0.2, 0.2)
        z = -np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.2)])
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        centre = -10.0 * z
        K = np.array([[rng.uniform(800, 1200), 0, 480], [0, rng.uniform(800, 1200), 240], [0, 0, 1]])
        P[c] = K @ np.concatenate([R, (-R @ centre)[:, None]], 1)
        centres[c] = centre
    X = rng.normal(0, 1.0, (T, J, 3))
    behind = rng.random((T, J)) < 0.05
    behind[0, 0] = True
    for t, j in np.argwhere(behind):   # behind camera 0, and at a depth of more than 0.5 for every camera (w = depth)
        while True:
            X[t, j] = centres[0] * rng.uniform(1.5, 3.0) + rng.normal(0, 0.1, 3)
            w = P[:, 2] @ np.append(X[t, j], 1.0)
            if w[0] < 0 and np.abs(w).min() > 0.5:
                break
    px = np.zeros((ncam, T, J, 2))
    for c in range(ncam):
        h = np.einsum("kl,tjl->tjk", P[c], np.concatenate([X, np.ones((T, J, 1))], -1))
        px[c, ..., 0] = h[..., 1] / h[..., 2] + rng.normal(0, 20, (T, J))
        px[c, ..., 1] = h[..., 0] / h[..., 2] + rng.normal(0, 20, (T, J))
    nview = rng.integers(0, 4, (T, J))
    nview[rng.random((T, J)) < 0.3] = ncam
    nview[0, 0] = ncam
    for t in range(T):
        for j in range(J):
            off = rng.permutation(ncam)[nview[t, j]:]
            px[off, t, j] = 0.0
            if (t, j) != (0, 0) and rng.random() < 0.1:   # one zero coordinate: not a view
                px[rng.integers(ncam), t, j, rng.integers(2)] = 0.0
    return P, px, X


@pytest.mark.parametrize("ncam", [2, 7, 8])
@pytest.mark.parametrize("J", [1, 19, 38, 64])
def test_sweep_with_poisoned_outputs(native_lib, cuda, ncam, J):
    rng = np.random.default_rng(100 * ncam + J)
    dp = ctypes.POINTER(ctypes.c_double)
    seen = set()
    for T in (1, 7, 37):   # never a multiple of the 4 frames of a block past T = 1
        P, px, X = _random_problem(rng, ncam, T, J)
        thr = rng.uniform(0, 60, J)
        thr[rng.random(J) < 0.2] = 0.0
        thr[rng.random(J) < 0.2] = np.inf
        if T == 7:
            thr[0] = 40.0   # frame 0 joint 0 is behind camera 0: flagged
        want = ro.reproj_errors(P, px, X, thr)
        seen |= {"flag"} if (want[2] != 0).any() else set()
        seen |= {"inf"} if np.isinf(want[0]).any() else set()
        seen |= {"zero"} if (want[0] == 0).any() else set()
        seen |= {"finite"} if (np.isfinite(want[0]) & (want[0] > 0)).any() else set()
        pxd, Xd = _dev(cuda, px, X)
        for with_jmax in (True, False):
            err = torch.full((ncam, T, J), float("nan"), dtype=torch.float64, device=cuda)
            jmax = torch.full((T, J), float("nan"), dtype=torch.float64, device=cuda)
            mask = torch.full((T,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=cuda)
            Ph, th = np.ascontiguousarray(P), np.ascontiguousarray(thr)
            rc = native_lib.df3d_reproj_errors(Ph.ctypes.data_as(dp), pxd.data_ptr(), Xd.data_ptr(), ncam, T, J, th.ctypes.data_as(dp), err.data_ptr(),
                                               jmax.data_ptr() if with_jmax else None, mask.data_ptr(), None)
            assert rc == 0
            torch.cuda.synchronize()
            if with_jmax:
                _compare((err, jmax, mask), want, thr)
            else:
                assert torch.isnan(jmax).all()
                _compare((err, want[1], mask), want, thr)
    assert seen == {"flag", "inf", "zero", "finite"}


def test_frames_selection_equals_the_full_rows(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops

    b = np.load(f"{golden_dir}/triangulate_bits.npz")
    px, X = _dev(cuda, b["random_px"], b["random_X"])
    thr = np.full(38, 25.0)
    frames = [5, 0, 31, 3, 3, 17]
    for given in (None, X):
        full = ops.reprojection_errors(b["P"], px, X=given, thresholds=thr)
        sel = ops.reprojection_errors(b["P"], px, X=given, thresholds=thr, frames=frames)
        assert torch.equal(sel[0], full[0][:, frames]) and torch.equal(sel[1], full[1][frames]) and torch.equal(sel[2], full[2][frames])
    empty = ops.reprojection_errors(b["P"], px, frames=[])
    assert [tuple(t.shape) for t in empty] == [(7, 0, 38), (0, 38), (0,)]
    with pytest.raises(IndexError):
        ops.reprojection_errors(b["P"], px, frames=[32])


PLANTED = [(0, 2, 0), (3, 10, 1), (7, 22, 2), (11, 30, 0), (14, 5, 2), (9, 25, 1)]   # (frame, joint, a-th view): three-view joints


def _plant(px, planted=PLANTED):
    """+100 px along the rows in one view of each planted joint (pixels [7, T, 38, 2])."""
    q = px.copy()
    for t, j, a in planted:
        views = np.flatnonzero((px[:, t, j] != 0).all(-1))
        assert len(views) == 3
        q[views[a], t, j, 0] += 100.0
    return q


def test_planted_outliers_change_exactly_those_flags(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import REPROJ_THR

    P, g3 = _cams(golden_dir)
    px = g3["points2d"] * HW
    (pxd,) = _dev(cuda, px)
    clean = ro.reproj_errors(P, px, ops.triangulate(P, pxd).cpu().numpy(), REPROJ_THR)
    want = ro.flags(clean[2], 38)
    for t, j, _ in PLANTED:
        assert not want[t, j]
        want[t, j] = True
    (qd,) = _dev(cuda, _plant(px))
    _, _, mask = ops.reprojection_errors(P, qd)   # X: the triangulation of the planted detections
    assert np.array_equal(ro.flags(mask.cpu().numpy(), 38), want)


# ------------------------------------------------------------------------------------------------------------------ Core
def _folder(tmp_path, golden_dir, T=15):
    """An input folder of T frames (every frame links to the sample's frame 0 of its camera)."""
    folder = tmp_path / "working"
    folder.mkdir()
    for c in range(7):
        for t in range(T):
            os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
    return str(folder)


def _resumed_core(folder, golden_dir, points2d):
    """A Core resumed from a result pickle holding the golden cameras and the given (normalised) detections."""
    from deepfly3d_amd.core import Core

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    out_dir = folder + "_df3d"
    os.makedirs(out_dir, exist_ok=True)
    pkl = os.path.join(out_dir, "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
    res = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "distort": g3["distort"][c], "intr": g3["intr"][c]} for c in range(7)}
    res.update(points2d=points2d, camera_ordering=g3["camera_ordering"], heatmap_confidence=g3["heatmap_confidence"])
    with open(pkl, "wb") as f:
        pickle.dump(res, f)
    core = Core(folder, out_dir, num_images_max=0, camera_ordering=ORDER)
    assert core.save_path == pkl and core.has_calibration and core.max_img_id == points2d.shape[1] - 1
    return core


def test_core_error_navigation_end_to_end(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import REPROJ_THR, config

    config.pop("image_shape", None)
    P, g3 = _cams(golden_dir)
    core = _resumed_core(_folder(tmp_path, golden_dir), golden_dir, _plant(g3["points2d"] * HW) / HW)
    px = core.camNet.points2d.copy()
    (pxd,) = _dev(cuda, px)
    err, jmax, mask = ro.reproj_errors(P, px, ops.triangulate(P, pxd).cpu().numpy(), REPROJ_THR)
    fl = ro.flags(mask, 38)
    bad = sorted({int(t) for t in np.flatnonzero(fl.any(1))})
    assert set(t for t, _, _ in PLANTED) <= set(bad)
    for i in range(-1, 16):
        assert core.next_error(i) == next((t for t in bad if t > i), None), i
        assert core.prev_error(i) == next((t for t in reversed(bad) if t < i), None), i
    assert core.next_error_in_range([1, 8, 7, 3, 14]) == 7
    for t in range(15):
        for j in range(0, 38, 3):
            assert core.joint_has_error(t, j) == fl[t, j]
        assert abs(core.get_joint_reprojection_error(t, 22) - jmax[t, 22]) <= ATOL
        assert abs(core.get_joint_reprojection_error(t, 22, camNet=[4, 5]) - err[4:6, t, 22].max()) <= ATOL
    _compare((core.reprojection_errors(), jmax, mask), (err, jmax, mask), REPROJ_THR)
    # a manual correction restoring frame 7's planted view: written into the camera network, it changes the answer
    t, j, a = PLANTED[2]
    c = int(np.flatnonzero((px[:, t, j] != 0).all(-1))[a])
    fixed = px[c, t].copy()
    fixed[j, 0] -= 100.0
    core.db.write(fixed / np.array(config["image_shape"]), c, t, True, [j])
    core.corrected_points2d_matrix()
    assert not core.joint_has_error(t, j)
    after = [b for b in bad if b != t or fl[t].sum() > 1]
    assert core.next_error(t - 1) == next(b for b in after if b > t - 1) and core.next_error(t - 1) != t
    config.pop("image_shape", None)


# ------------------------------------------------------------------------------------------------------------------ flagged-only correction
def test_auto_correct_flagged_only_keeps_unflagged_argmax(native_lib, cuda, tmp_path, golden_dir):
    """The planted-distractor scenario of test_gpu_pictorial.py: distractor peaks in one camera of many joints pull the arg-max
    detections away.  flagged_only=True keeps the full correction on the flagged joints and the arg-max detection elsewhere."""
    import test_gpu_pictorial as tgp

    from deepfly3d_amd import ops
    from deepfly3d_amd.config import REPROJ_THR, config

    config.pop("image_shape", None)
    P, hm, cell = tgp._render(golden_dir)
    T = hm.shape[1]
    rng = np.random.default_rng(11)
    import pictorial_oracle as po

    table = po.seeing_table(ORDER)
    for t in range(T):
        for j in rng.choice(38, 12, replace=False):
            c, src, _ = table[j][int(rng.integers(len(table[j])))]
            r0, c0 = cell[(c, t, j)]
            while True:
                rd, cd = int(rng.integers(2, 62)), int(rng.integers(2, 126))
                if (rd - r0) ** 2 + (cd - c0) ** 2 >= 20**2:
                    break
            hm[c, t, src] = np.maximum(hm[c, t, src], tgp._gauss(rd, cd, h=1.3))
    am, _, _, _, (count, pts, vals) = tgp._run(P, hm, cuda)
    folder = _folder(tmp_path, golden_dir, T)
    full = _resumed_core(folder, golden_dir, am.cpu().numpy())
    full.peaks = tuple(x.cpu().numpy() for x in (count, pts, vals))
    full.auto_correct()
    part = _resumed_core(folder, golden_dir, am.cpu().numpy())
    part.peaks = full.peaks
    part.auto_correct(flagged_only=True)
    # the flags: the arg-max detections at the arg-max DLT point, on the Core's cameras
    P = np.stack([c.P for c in part.camNet.cam_list])
    X0 = ops.arg_max_points3d(P, am, [960, 480])
    scale = torch.tensor(HW, device=cuda)
    _, _, mask = ops.reprojection_errors(P, (am * scale).contiguous(), X=X0)
    fl = ro.flags(mask.cpu().numpy(), 38)
    amh = am.cpu().numpy()
    want = ro.reproj_errors(P, amh * HW, X0.cpu().numpy(), REPROJ_THR)
    near = np.abs(want[1] - REPROJ_THR) <= NEAR
    assert np.array_equal(fl[~near], ro.flags(want[2], 38)[~near])
    changed = (full.points2d != amh).any(-1).any(0)
    assert fl.sum() > 0 and (changed & fl).any() and (changed & ~fl).any()
    assert np.array_equal(part.points2d[:, ~fl], amh[:, ~fl])
    assert np.array_equal(part.points2d[:, fl], full.points2d[:, fl])
    assert np.array_equal(part.points2d_argmax, amh) and np.array_equal(part.camNet.points2d, part.points2d * HW)
    config.pop("image_shape", None)


def _cli(launcher, folder, env, root):
    r = subprocess.run(launcher + [folder, "-n", "2", "-vv", "--auto-correct", "--correct-only-flagged"], env=env, cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "flagged joints" in r.stdout
    files = [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]
    assert len(files) == 1
    with open(os.path.join(folder + "_df3d", files[0]), "rb") as f:
        return pickle.load(f)


def test_cli_correct_only_flagged_two_ranks_match_one_rank(native_lib, cuda, tmp_path, golden_dir):
    from oracle import geometry as og

    from deepfly3d_amd import ops

    import test_gpu_pictorial as tgp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DF3D_SYNTHETIC_WEIGHTS="0", DF3D_DIST_BACKEND="gloo", PYTHONPATH=root)
    results = []
    for tag, launcher in (("one", [sys.executable, "-m", "deepfly3d_amd.cli"]),
                          ("two", [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                   "--master-port", "29641", "-m", "deepfly3d_amd.cli"])):
        base = tmp_path / tag
        base.mkdir()
        results.append(_cli(launcher, tgp._sample_folder(base, golden_dir), env, root))
    one, two = results
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    assert [str(k) for k in one.keys()] == [str(k) for k in g3["key_order"]] + ["points2d_argmax"]
    assert list(one.keys()) == list(two.keys())
    for k in ("points2d", "points2d_argmax", "heatmap_confidence", "camera_ordering"):
        assert np.array_equal(one[k], two[k]), k
    assert np.allclose(one["points3d_wo_procrustes"], two["points3d_wo_procrustes"], atol=1e-9)
    # unflagged joints keep their arg-max detections
    P = og.projection_matrices(*(np.stack([one[c][n] for c in range(7)]) for n in ("R", "tvec", "intr")))
    (am,) = _dev(cuda, one["points2d_argmax"])
    _, _, mask = ops.reprojection_errors(P, (am * torch.tensor(HW, device=cuda)).contiguous(), X=ops.arg_max_points3d(P, am, [960, 480]))
    fl = ro.flags(mask.cpu().numpy(), 38)
    assert np.array_equal(one["points2d"][:, ~fl], one["points2d_argmax"][:, ~fl])
