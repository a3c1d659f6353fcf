"""-m gpu tests of the consensus triangulation (csrc/consensus.hip).  The candidates' points meet the SVD oracle
under the project's DLT bar; everything after them -- errors, choice, status, replaced detections, counts -- equals
tests/consensus_oracle.py exactly when the oracle is given the device's own candidate points (teacher-forced)."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import consensus_cases as cc
import consensus_oracle as co
import pose_chain_cases as pc

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the cached cases are read-only


def _host(r):
    return tuple(v.cpu().numpy() for v in (r.points3d, r.cameras, r.status, r.error, r.fixed_px, r.counts))


def _same(got, want, what):
    for name, g, w in zip(("X", "cameras", "status", "err", "fixed_px", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w, equal_nan=True), (what, name, int((g != w).sum()))


def _teacher_forced(ops, P, px, cuda, tau, min_views=2, check_q=True):
    """The fused entry against the oracle on the device's candidate points; returns the device's outputs."""
    d = _dev(px, cuda)
    full = ops.triangulate(P, d)
    cand_X, cand_q = ops.consensus_candidates(P, d, full)
    got = _host(ops.triangulate_consensus(P, d, full, tau=tau, min_views=min_views))
    cand = cand_X.cpu().numpy()
    _same(got, co.choose(P, px, cand, full.cpu().numpy(), tau, min_views), (px.shape, tau, min_views))
    if check_q:
        assert np.array_equal(cand_q.cpu().numpy(), co.squared_errors(P, px, cand), equal_nan=True)
    return got


def test_candidates_meet_the_svd_oracle(native_lib, cuda):
    """All 247 subsets of the eight cameras on the 300 clean detections, bar TRI_BAR (the condition: tests/test_consensus_host.py)."""
    from deepfly3d_amd import ops

    P, px = cc.rig(), pc.detections()[0]
    d = _dev(px, cuda)
    full = ops.triangulate(P, d)
    cand_X, cand_q = (t.cpu().numpy() for t in ops.consensus_candidates(P, d))
    assert cand_X.shape == (300, 1, 256, 3) and cand_q.shape == (300, 1, 256, 8)
    want = co.candidates(P, px)
    size = np.array([bin(m).count("1") for m in range(256)])
    worst = {int(k): float(np.abs(cand_X[:, :, (size == k) & (np.arange(256) != 255)] - want[:, :, (size == k) & (np.arange(256) != 255)]).max())
             for k in range(2, 8)}
    worst[8] = float(np.abs(cand_X[:, :, 255] - want[:, :, 255]).max())
    print("worst |device - SVD| by subset size: " + ", ".join(f"{k}: {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= pc.TRI_BAR
    assert not cand_X[:, :, size < 2].any() and not cand_q[:, :, size < 2].any()
    assert np.array_equal(cand_X[:, :, 255], full.cpu().numpy())           # the all-views entry is the caller's point
    member = (np.arange(256)[:, None] >> np.arange(8)) & 1
    assert not cand_q[:, :, member == 0].any() and (cand_q[:, :, (member == 1) & (size[:, None] >= 2)] > 0).all()
    assert np.array_equal(cand_q, co.squared_errors(P, px, cand_X))


def test_candidates_of_packed_launches_meet_the_svd_oracle(native_lib, cuda):
    """The launches whose points differ in their number of views, so that points of several group sizes share a block and a pass: the
    candidates' points of their clean variants against the SVD of each subset, bar TRI_BAR (the condition:
    tests/test_consensus_host.py).  A contribution or a lane that the packing misplaced would move a point here."""
    from deepfly3d_amd import ops

    for name, P, px in cc.packed_clean_cases():
        cand_X = ops.consensus_candidates(P, _dev(px, cuda))[0].cpu().numpy()
        want = co.candidates(P, px)       # the all-views entry included: there the device holds df3d_triangulate's point
        worst = float(np.abs(cand_X - want).max())
        print(f"{name}: worst |device - SVD| {worst:.1e} over {int((want != 0).any(axis=-1).sum())} candidates")
        assert worst <= pc.TRI_BAR and np.array_equal(cand_X != 0, want != 0), name


@pytest.mark.parametrize("ncam,T,J", [(2, 1, 1), (3, 1, 1), (3, 255, 1), (3, 256, 1), (3, 257, 1), (2, 3, 64), (7, 5, 13), (8, 33, 1), (8, 3, 11)])
def test_the_choice_is_the_oracles_on_the_devices_points(native_lib, cuda, ncam, T, J):
    """Point counts round the 32-point block and the 256-lane pass, two to eight cameras, J up to 64: a third of the points carry an
    outlier, a third miss a camera."""
    from deepfly3d_amd import ops

    px = cc.mixed(ncam, T, J)
    tau = np.linspace(3.0, 8.0, J)
    X, cameras, status, err, fixed, counts = _teacher_forced(ops, cc.rig(ncam), px, cuda, tau)
    assert counts.sum() == T * J
    if T * J >= 33 and ncam >= 3:
        assert (status == 1).any() and (status == 2).any()


def test_consecutive_points_of_zero_to_eight_views(native_lib, cuda):
    """One launch in which the points see 0, 1, 2, ... 8 views in turn: every group size packs into the same passes."""
    from deepfly3d_amd import ops

    P, px = cc.rig(), cc.staircase()
    for min_views in (2, 3, 8):
        X, cameras, status, err, fixed, counts = _teacher_forced(ops, P, px, cuda, cc.TAU, min_views)
        n = np.array([bin(co.view_mask(px[:, i, 0])).count("1") for i in range(px.shape[1])])
        assert np.array_equal(status[:, 0] == 0, n < 2)
        assert np.isin(status[n < min_views, 0], (0, 3)).all()
    # the same points as [T, J] = [9, 3] and as J = 27 of one frame
    for T, J in ((9, 3), (1, 27)):
        _teacher_forced(ops, P, np.ascontiguousarray(px.reshape(8, T, J, 2)), cuda, cc.TAU)


def test_the_fly_layout(native_lib, cuda):
    """ncam 7, J 38, the visibility of config.camera_see_joint, T = 40."""
    from deepfly3d_amd import ops

    px, see = cc.fly_layout()
    X, cameras, status, err, fixed, counts = _teacher_forced(ops, cc.rig(7), px, cuda, np.full(38, cc.TAU))
    views = see.sum(axis=0)
    assert views.max() == 4 and set(np.unique(views)) <= {0, 2, 3, 4}
    assert np.array_equal(status == 0, np.broadcast_to(views < 2, status.shape))
    assert (status == 2).sum() >= 40 * 38 // 10 and counts.sum() == 40 * 38
    hidden = ~np.broadcast_to(see[:, None, :], err.shape)
    assert not err[hidden].any() and not fixed[hidden].any()


def test_infinite_and_zero_tau(native_lib, cuda):
    from deepfly3d_amd import ops

    P, px = cc.rig(), cc.staircase()
    d = _dev(px, cuda)
    full = ops.triangulate(P, d)
    n = np.array([bin(co.view_mask(px[:, i, 0])).count("1") for i in range(px.shape[1])])
    r = ops.triangulate_consensus(P, d, tau=math.inf)
    assert torch.equal(r.points3d, full) and np.array_equal(r.status.cpu().numpy()[:, 0], np.where(n >= 2, 1, 0))
    assert torch.equal(r.fixed_px, d)
    r = ops.triangulate_consensus(P, d, tau=0.0)
    assert torch.equal(r.points3d, full) and np.array_equal(r.status.cpu().numpy()[:, 0], np.where(n >= 2, 3, 0))
    assert torch.equal(r.fixed_px, d) and r.params[0].tolist() == [0.0] and r.params[1] == 2
    _teacher_forced(ops, P, px, cuda, math.inf)
    _teacher_forced(ops, P, px, cuda, 0.0)


def test_behind_a_camera_and_non_finite_detections(native_lib, cuda):
    """Camera 2's matrix is negated: the DLT does not notice, w < 0 does, so no chosen set holds it.  A NaN or an infinity in a
    detection leaves status 3 or a subset without that camera, as the oracle says."""
    from deepfly3d_amd import ops

    P, px = cc.special()
    X, cameras, status, err, fixed, counts = _teacher_forced(ops, P, px, cuda, cc.TAU)
    assert not (cameras[status != 3] >> 2 & 1).any()
    assert (status[:8, 0] == 2).all() and (cameras[:8, 0] == 0b11111011).all() and np.isinf(err[2, :8, 0]).all()
    assert (status[8:12, 0] == 3).all() and (cameras[8:12, 0] == 0b100100).all()          # its only partner is behind: nothing qualifies
    assert (status[12:16, 0] == 2).all() and (cameras[12:16, 0] == 0b100010).all()
    bad = ~np.isfinite(px).all(axis=-1)[:, :, 0]                                            # [8, 24]
    assert bad[:, 16:].any(axis=0).all()
    assert (status[16:, 0] == 2).all() and not ((cameras[16:, 0][None] >> np.arange(8)[:, None] & 1).astype(bool) & bad[:, 16:]).any()
    assert np.isfinite(X[16:]).all() and np.isinf(err[:, 16:, 0][bad[:, 16:]]).all()
    assert np.isfinite(fixed[:, 16:, 0][bad[:, 16:]]).all()                                # the rejected NaN detections are replaced


def test_planted_outliers_are_rejected(native_lib, cuda):
    """The production path alone, no teacher: the clean camera set of every point of the layouts with at least three clean views."""
    from deepfly3d_amd import ops

    for layout in cc.CLEAN_LAYOUTS:
        px, clean = cc.planted(*layout)
        r = ops.triangulate_consensus(cc.rig(), _dev(px, cuda), tau=cc.TAU)
        assert np.array_equal(r.cameras.cpu().numpy()[:, 0], clean), layout
        assert (r.status == 2).all() and r.counts.cpu().numpy().tolist() == [[0, 0, 300, 0]]


def test_two_runs_give_the_same_bits_and_the_counts_add_up(native_lib, cuda):
    from deepfly3d_amd import ops

    px = cc.mixed(7, 600, 38, seed=1)     # three count slices of 256 frames
    d, P = _dev(px, cuda), cc.rig(7)
    a, b = ops.triangulate_consensus(P, d, tau=cc.TAU), ops.triangulate_consensus(P, d, tau=cc.TAU)
    for x, y in zip(_host(a), _host(b)):
        assert x.tobytes() == y.tobytes()
    status = a.status.cpu().numpy()
    want = np.stack([(status == s).sum(axis=0) for s in range(4)], axis=1)
    assert np.array_equal(a.counts.cpu().numpy(), want) and a.counts.dtype == torch.int64 and want[:, 1].sum() > 0 and want[:, 2].sum() > 0
    empty = ops.triangulate_consensus(P, d[:, :0].contiguous())
    assert tuple(empty.points3d.shape) == (0, 38, 3) and tuple(empty.fixed_px.shape) == (7, 0, 38, 2) and not empty.counts.any()
    with pytest.raises(ValueError, match="tau must hold one value, or one per joint"):
        ops.triangulate_consensus(P, d, tau=[1.0, 2.0])
    with pytest.raises(ValueError, match="X must be"):
        ops.triangulate_consensus(P, d, X=torch.zeros((600, 38, 2), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="must not overlap"):
        _native_overlap(ops, P, d)


def _native_overlap(ops, P, d):
    """The fused entry refuses an output that shares bytes with an input."""
    import ctypes

    from deepfly3d_amd import _native

    ncam, T, J, _ = d.shape
    full = ops.triangulate(P, d)
    lib = _native.load()
    t = np.full(J, 5.0)
    out = [torch.empty(s, dtype=k, device=d.device) for s, k in (((T, J), torch.int32), ((T, J), torch.int8), ((ncam, T, J), torch.float64))]
    need = lib.df3d_consensus_work_bytes(ncam, T, J)
    work = torch.empty(need, dtype=torch.uint8, device=d.device)
    dp = ctypes.POINTER(ctypes.c_double)
    ops._call("df3d_triangulate_consensus", np.ascontiguousarray(P).ctypes.data_as(dp), d.data_ptr(), full.data_ptr(), ncam, T, J,
              t.ctypes.data_as(dp), 2, full.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None, None, work.data_ptr(),
              need, ops._stream(d))


# ------------------------------------------------------------------------------------------------------------------ Core
def _recording(tmp_path, golden_dir):
    """(folder, result pickle): 15 frames (links to the sample's frame 0) and an earlier result holding the golden detections and cameras."""
    folder = tmp_path / "working"
    folder.mkdir()
    for c in range(7):
        for t in range(15):
            os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
    folder = str(folder)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    os.makedirs(folder + "_df3d")
    pkl = os.path.join(folder + "_df3d", "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
    res = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "distort": g3["distort"][c], "intr": g3["intr"][c]} for c in range(7)}
    res.update(points2d=g3["points2d"], camera_ordering=g3["camera_ordering"], heatmap_confidence=g3["heatmap_confidence"])
    with open(pkl, "wb") as f:
        pickle.dump(res, f)
    return folder, pkl


def _load(pkl):
    with open(pkl, "rb") as f:
        return pickle.load(f)


def _same_value(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same_value(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_core_saves_the_robust_pose(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    core.save()
    plain = _load(pkl)
    assert not any("robust" in str(k) for k in plain)
    core.save(robust_triangulation=True)
    run = _load(pkl)
    assert list(run) == list(plain) + list(Core._ROBUST_KEYS) and len(Core._ROBUST_KEYS) == 7
    assert all(_same_value(run[k], plain[k]) for k in plain)
    T = plain["points2d"].shape[1]
    assert run["points3d_robust"].shape == (T, 38, 3) and run["robust_cameras"].shape == (T, 38) and run["robust_cameras"].dtype == np.int32
    assert run["robust_status"].dtype == np.int8 and run["robust_error"].shape == (7, T, 38) and run["robust_counts"].shape == (38, 4)
    assert run["points2d_robust"].shape == (7, T, 38, 2) and run["robust_counts"].sum() == T * 38
    assert np.array_equal(run["robust_params"], np.append(cfg.ROBUST_TAU, 2.0))
    # what the method returns, and what the oracle says on the device's candidate points
    r = core.robust_triangulation()
    assert isinstance(r, ops.ConsensusResult) and all(isinstance(v, np.ndarray) for v in (r.points3d, r.cameras, r.status, r.error, r.fixed_px, r.counts))
    for key, value in zip(Core._ROBUST_KEYS[:5], (r.points3d, r.cameras, r.status, r.error, r.counts)):
        assert _same_value(run[key], value), key
    px = np.ascontiguousarray(core.camNet.points2d, dtype=np.float64)
    assert _same_value(run["points2d_robust"], r.fixed_px / np.asarray(core.image_shape[::-1], dtype=np.float64))
    P = np.stack([c.P for c in core.camNet.cam_list])
    got = _teacher_forced(ops, P, px, cuda, cfg.ROBUST_TAU, check_q=False)
    assert _same_value(got[0], r.points3d) and _same_value(got[1], r.cameras)
    where1 = run["robust_status"] == 1
    assert where1.any() and np.array_equal(run["points3d_robust"][where1], plain["points3d_wo_procrustes"][where1])
    print(f"the golden recording: status counts {run['robust_counts'].sum(axis=0).tolist()}")
    # the other keys of the same save come from the robust pose; with repair_pose it is repaired afterwards
    other = core.robust_triangulation(tau=2.0, min_views=2)
    core.save(joint_angles=True, repair_pose=True, robust_triangulation=True, robust_tau=2.0)
    run = _load(pkl)
    assert list(run) == list(plain) + ["joint_angles", "segment_lengths"] + list(Core._REPAIR_KEYS) + list(Core._ROBUST_KEYS)
    assert all(_same_value(run[k], plain[k]) for k in plain) and _same_value(run["points3d_robust"], other.points3d)
    repaired = ops.repair_pose(_dev(other.points3d, cuda))
    assert _same_value(run["points3d_repaired"], repaired.points.cpu().numpy())
    angles = ops.joint_angles(repaired.points)[0].cpu().numpy()
    assert np.array_equal(run["joint_angles"], angles, equal_nan=True)
    core.save(joint_angles=True, robust_triangulation=True, robust_tau=2.0)
    run = _load(pkl)
    assert list(run) == list(plain) + ["joint_angles", "segment_lengths"] + list(Core._ROBUST_KEYS)
    angles = ops.joint_angles(_dev(run["points3d_robust"], cuda))[0].cpu().numpy()
    assert np.array_equal(run["joint_angles"], angles, equal_nan=True)
    # a detection moved by 60 px.  The re-layout gives the front camera no joint, so no joint of this rig has four views: three are
    # used, where the model cannot always tell, and only equality with the oracle is asserted
    views = (px != 0.0).all(axis=-1)
    assert views.sum(axis=0).max() == 3
    j = int(np.nonzero(views[:, 0].sum(axis=0) == 3)[0][0])
    cam = int(np.nonzero(views[:, 0, j])[0][0])
    before = core.camNet.points2d[cam, 0, j].copy()
    core.camNet.points2d[cam, 0, j] += (0.0, cc.OUTLIER_PX)
    moved = np.ascontiguousarray(core.camNet.points2d[:, :1], dtype=np.float64)
    want = _teacher_forced(ops, P, moved, cuda, cfg.ROBUST_TAU, check_q=False)
    rejected = {jj: [c for c in range(7) if views[c, 0, jj] and want[2][0, jj] == 2 and not want[1][0, jj] >> c & 1] for jj in range(38)}
    assert core.outlier_cameras(0, j) == rejected[j]
    assert core.outlier_cameras(0) == {jj: cams for jj, cams in rejected.items() if cams}
    print(f"joint {j}, camera {cam} moved by 60 px: status {int(want[2][0, j])}, rejected {rejected[j]}")
    core.camNet.points2d[cam, 0, j] = before
    with pytest.raises(IndexError):
        core.outlier_cameras(T)
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_robust_triangulation(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    order = [str(c) for c in range(7)]
    assert cli.main([folder, "--skip-pose-estimation", "--robust-triangulation", "--robust-tau", "7.5", "--robust-min-views", "3", "--order"] + order) == 0
    run = _load(pkl)
    assert list(run)[-7:] == list(Core._ROBUST_KEYS) and run["robust_params"].tolist() == [7.5] * 38 + [3.0]
    assert not (run["robust_status"] == 2).any()   # at most three views: a proper subset holds fewer than min_views
    assert run["points3d_robust"].shape == run["points3d_wo_procrustes"].shape
    config.pop("image_shape", None)
