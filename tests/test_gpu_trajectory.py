"""-m gpu tests of the trajectory triangulation (csrc/trajectory.hip).  The linearisation equals
tests/trajectory_oracle.py bit for bit; the banded solve meets a backward-error bar set by the oracle's own float64 factorisation; the
whole fit agrees with the oracle exactly in everything discrete and, in the points, within a bar measured from the oracle's own
sensitivity to rounding (float64 against numpy.longdouble)."""
import os
import pickle

import numpy as np
import pytest
import torch

import consensus_cases as cc
import trajectory_cases as tc
import trajectory_oracle as to
from deepfly3d_amd import config

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the cached cases are read-only


# ---------------------------------------------------------------------------------------------------------------------- linearise
def _linearize_cases():
    P8, special = cc.special()
    return [("fly layout", cc.rig(7), cc.fly_layout()[0]), ("mixed 8 x 5 x 13", cc.rig(8), cc.mixed(8, 5, 13)),
            ("special", P8, np.ascontiguousarray(special))]


@pytest.mark.parametrize("delta", [10.0, 2.0, 0.0, np.inf])
def test_linearize_is_bit_exact(native_lib, cuda, delta):
    """H, g, weights, errors and the chains' costs at the device's own triangulation and at a point 0.05 mm beside it."""
    from deepfly3d_amd import ops

    for name, P, px in _linearize_cases():
        d = _dev(px, cuda)
        for shift in (0.0, 0.05):
            X = ops.triangulate(P, d) + shift
            got = [t.cpu().numpy() for t in ops.trajectory_linearize(P, d, X, huber=delta)]
            want = to.linearize(P, px, X.cpu().numpy(), delta)
            want = want[:4] + (to.chain_sum(want[4]),)
            for what, g, w in zip(("H", "g", "weight", "error", "cost"), got, want):
                assert g.shape == w.shape and g.dtype == w.dtype, (name, what)
                assert np.array_equal(g, w, equal_nan=True), (name, delta, shift, what, int((g != w).sum()))
        if name == "special":   # points behind a camera and non-finite detections are views of weight 0 and infinite error
            assert np.isinf(got[3]).any() and (got[2][np.isinf(got[3])] == 0.0).all()


def test_linearize_chain_sum_crosses_the_lanes(native_lib, cuda):
    """257 and 513 frames: a lane adds two and three frames before the tree."""
    from deepfly3d_amd import ops

    for T in (257, 513):
        P, px = tc.clean(3, T, 2)[:2]
        X = _dev(tc.dlt(P, px), cuda)
        got = ops.trajectory_linearize(P, _dev(px, cuda), X, huber=tc.HUBER)[4].cpu().numpy()
        assert np.array_equal(got, to.chain_sum(to.linearize(P, px, X.cpu().numpy(), tc.HUBER)[4]))


# ---------------------------------------------------------------------------------------------------------------------- the solve
@pytest.mark.parametrize("lam", tc.SOLVE_LAMBDAS)
@pytest.mark.parametrize("J", [1, 38])
def test_banded_solve_meets_the_backward_error_bar(native_lib, cuda, J, lam):
    """Every block size at its lengths.  The bar: 8 x max(the oracle's own banded factorisation on the same system, eps)."""
    from deepfly3d_amd import ops

    worst, across = (0.0, 0.0), 0.0
    for T in sorted({T for B in tc.SOLVE_BLOCKS for T in tc.solve_lengths(B)}):
        for B in (B for B in tc.SOLVE_BLOCKS if T in tc.solve_lengths(B)):
            AB, b, seg, G = tc.solve_system(T, J, B, lam)
            H = tc.solve_terms(T, J)[0]
            d, ok = ops.trajectory_solve(_dev(H, cuda), _dev(G, cuda), _dev(seg, cuda), lam, tc.SOLVE_MU, block_frames=B)
            assert ok.cpu().numpy().all()
            d = d.cpu().numpy()
            assert not d[seg == 0].any()                       # a frame outside the segments does not move
            x = d.transpose(1, 0, 2).reshape(J, 3 * T)
            ref, ref_ok = to.banded_solve(AB, b)
            assert ref_ok.all()
            mine, theirs = to.backward_error(AB, b, x), to.backward_error(AB, b, ref)
            bar = 8.0 * np.maximum(theirs, EPS)
            print(f"J {J} lambda {lam:g} T {T} B {B}: device {mine.max():.2e} oracle {theirs.max():.2e}")
            assert (mine <= bar).all(), (T, B, float(mine.max()), float(theirs.max()))
            worst = max(worst, (float(mine.max()), float(theirs.max())))
        # one segment table for every block size (that of B = 7): the same system, and the answers agree within the same bar --
        # |A (x - y)| over the backward error's denominator, every pair of block sizes
        seg = tc.segment_table(T, J, 7)
        AB, b, _, G = tc.solve_system(T, J, 7, lam)
        ref = to.banded_solve(AB, b)[0]
        bar = 8.0 * np.maximum(to.backward_error(AB, b, ref), EPS)
        xs = []
        for B in tc.SOLVE_BLOCKS:
            d = ops.trajectory_solve(_dev(tc.solve_terms(T, J)[0], cuda), _dev(G, cuda), _dev(seg, cuda), lam, tc.SOLVE_MU, block_frames=B)[0]
            xs.append(d.cpu().numpy().transpose(1, 0, 2).reshape(J, 3 * T))
            assert (to.backward_error(AB, b, xs[-1]) <= bar).all(), (T, B)
        for k, x0 in enumerate(xs):
            for x1 in xs[k + 1:]:
                apart = to.backward_error(AB, b, x0, other=x1)
                across = max(across, float((apart / bar).max()))
                assert (apart <= bar).all(), (T, float(apart.max()), float(bar.min()))
    print(f"worst backward error, J {J} lambda {lam:g}: device {worst[0]:.2e} (oracle there {worst[1]:.2e}); "
          f"two block sizes apart by at most {across:.2f} of the bar")


# ---------------------------------------------------------------------------------------------------------------------- the fit
_reference, _error_and_cost_bars = tc.reference, tc.error_and_cost_bars   # shared with tests/test_gpu_trajectory_sweep.py


def _same_bits(a, b):
    """Two device tensors hold the same bits (a NaN equals itself here)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


@pytest.mark.parametrize("T", tc.FIT_LENGTHS)
@pytest.mark.parametrize("name", tc.FIT_CASES)
def test_whole_fit_against_the_oracle(native_lib, cuda, name, T):
    from deepfly3d_amd import ops

    P, px = tc.fit_case(name, T)
    d = _dev(px, cuda)
    X0 = ops.triangulate(P, d)
    r64, r80, moved, bar = _reference(P, px, X0.cpu().numpy())
    # the condition of the comparison, not a tolerance: the oracle converges on every chain, in both precisions
    assert (r64["fit_status"] == to.CONVERGED).all() and (r80["fit_status"] == to.CONVERGED).all()
    assert not (r64["status"] == 4).any()
    first, lam = None, config.TRAJECTORY_LAMBDA[: px.shape[2]]
    error_bar, cost_bar = _error_and_cost_bars(P, px, r64, lam, config.TRAJECTORY_HUBER, bar)
    for B in tc.FIT_BLOCKS:
        r = ops.triangulate_trajectory(P, d, X0, lam=lam, block_frames=B)
        X, status, weight = r.points3d.cpu().numpy(), r.status.cpu().numpy(), r.weight.cpu().numpy()
        assert np.array_equal(status, r64["status"]), (name, T, B)
        assert np.array_equal(r.counts.cpu().numpy(), r64["counts"])
        assert np.array_equal(weight < 1.0, r64["weight"] < 1.0), (name, T, B, int(((weight < 1.0) != (r64["weight"] < 1.0)).sum()))
        worst = float(np.abs(X - r64["X"]).max())
        print(f"{name} T {T} B {B}: |device - oracle| {worst:.2e}, float64 against longdouble {moved:.2e}, bar {bar:.2e}, "
              f"iterations {r.iterations.cpu().numpy().max()} (oracle {r64['iterations'].max()})")
        assert worst <= bar, (name, T, B, worst, bar)
        err, want = r.error.cpu().numpy(), r64["error"]
        finite = np.isfinite(want)
        assert np.array_equal(np.isfinite(err), finite) and np.array_equal(err == 0.0, want == 0.0)
        assert (np.abs(err - want)[finite] <= error_bar[finite]).all(), (name, T, B, float(np.abs(err - want)[finite].max()))
        cost = r.cost.cpu().numpy()
        assert np.array_equal(cost[:, 0], r64["cost"][:, 0])               # the start's cost: the oracle's operations, bit for bit
        assert (np.abs(cost[:, 1] - r64["cost"][:, 1]) <= cost_bar).all(), (name, T, B, np.abs(cost[:, 1] - r64["cost"][:, 1]).max(), cost_bar.min())
        again = ops.triangulate_trajectory(P, d, X0, lam=lam, block_frames=B)
        for what in ("points3d", "status", "weight", "error", "iterations", "cost", "counts"):
            assert _same_bits(getattr(r, what), getattr(again, what)), (name, T, B, what)   # two runs give the same bits
        if first is None:
            first = X
        assert float(np.abs(X - first).max()) <= bar


def test_limits(native_lib, cuda):
    """lambda = 0, delta = inf and max_gap = 0: a frame that is no anchor keeps its input, and an anchor moves as the per-point refinement
    of the oracle does.  T = 1 and T = 2 copy the input."""
    from deepfly3d_amd import ops

    P, px = tc.fit_case("gaps", 40)
    d = _dev(px, cuda)
    X0 = ops.triangulate(P, d)
    r = ops.triangulate_trajectory(P, d, X0, lam=0.0, huber=np.inf, max_gap=0)
    ref = to.fit(P, px, X0.cpu().numpy(), 0.0, np.inf, 0)
    ref80 = to.fit(P, px, X0.cpu().numpy(), 0.0, np.inf, 0, dtype=np.longdouble)
    assert (ref["fit_status"] == to.CONVERGED).all()
    status, X = r.status.cpu().numpy(), r.points3d.cpu().numpy()
    assert np.array_equal(status, ref["status"]) and set(np.unique(status)) == {0, 1}
    assert np.array_equal(X[status == 0], X0.cpu().numpy()[status == 0])
    bar = max(16.0 * float(np.abs(ref["X"] - ref80["X"].astype(np.float64)).max()), config.TRAJECTORY_STEP_TOL)
    assert float(np.abs(X - ref["X"]).max()) <= bar
    assert (r.weight.cpu().numpy()[:, status == 1][:3] == 1.0).all()          # delta = inf: plain least squares
    for T in (1, 2):
        short = d[:, :T].contiguous()
        r = ops.triangulate_trajectory(P, short, X0[:T].contiguous(), lam=0.0, huber=np.inf, max_gap=0)
        assert torch.equal(r.points3d, X0[:T]) and not r.status.any() and not r.weight.any() and not r.iterations.any()
        r = ops.triangulate_trajectory(P, short, X0[:T].contiguous(), lam=tc.LAMBDA)
        assert torch.equal(r.points3d, X0[:T]) and not r.status.any()
    r = ops.triangulate_trajectory(P, d[:, :0].contiguous(), X0[:0].contiguous(), lam=tc.LAMBDA)
    assert r.points3d.shape == (0, 2, 3) and r.counts.shape == (2, 5) and not r.counts.any()


def test_inactive_frames_keep_their_bits(native_lib, cuda):
    """A chain without an anchor, one with a single anchor, and a -0.0 and a NaN among the inputs of frames outside every segment."""
    from deepfly3d_amd import ops

    P, px = tc.fit_case("clean3", 40)
    px = np.array(px)
    px[:, :, 0] = 0.0                 # joint 0: no view at all
    px[1:, 5:, 1] = 0.0               # joint 1: anchors 0 .. 4, then one view only to the end (no anchor closes the run)
    X0 = np.array(tc.dlt(P, px))
    X0[:, 0] = (-0.0, np.nan, 3.0)
    r = ops.triangulate_trajectory(P, _dev(px, cuda), _dev(X0, cuda), lam=tc.LAMBDA)
    ref = to.fit(P, px, X0, config.TRAJECTORY_LAMBDA[:2], config.TRAJECTORY_HUBER, config.REPAIR_MAX_GAP)
    status, X = r.status.cpu().numpy(), r.points3d.cpu().numpy()
    assert np.array_equal(status, ref["status"]) and not status[:, 0].any() and status[:5, 1].all() and not status[5:, 1].any()
    assert np.array_equal(X[status == 0].view(np.int64), X0[status == 0].view(np.int64))
    assert np.array_equal(r.counts.cpu().numpy(), ref["counts"])


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


def _counted(monkeypatch, ops, name):
    calls, inner = [], getattr(ops, name)

    def wrapper(*args, **kw):
        calls.append(name)
        return inner(*args, **kw)

    monkeypatch.setattr(ops, name, wrapper)
    return calls


def test_core_saves_the_trajectory_pose(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config as settings
    from deepfly3d_amd.core import Core

    settings.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    core.save()
    plain = _load(pkl)
    assert not any("trajectory" in str(k) for k in plain)
    fits, votes = _counted(monkeypatch, ops, "triangulate_trajectory"), _counted(monkeypatch, ops, "triangulate_consensus")
    core.save(trajectory_triangulation=True)
    run = _load(pkl)
    assert list(run) == list(plain) + list(Core._TRAJECTORY_KEYS) and len(Core._TRAJECTORY_KEYS) == 8
    assert all(_same_value(run[k], plain[k]) for k in plain) and fits == ["triangulate_trajectory"] and not votes
    T = plain["points2d"].shape[1]
    assert run["points3d_trajectory"].shape == (T, 38, 3) and run["trajectory_status"].shape == (T, 38) and run["trajectory_status"].dtype == np.int8
    assert run["trajectory_weight"].shape == (7, T, 38) and run["trajectory_error"].shape == (7, T, 38)
    assert run["trajectory_iterations"].shape == (38,) and run["trajectory_iterations"].dtype == np.int32
    assert run["trajectory_cost"].shape == (38, 2) and run["trajectory_counts"].shape == (38, 5) and run["trajectory_counts"].sum() == T * 38
    assert np.array_equal(run["trajectory_params"], np.append(config.TRAJECTORY_LAMBDA, [config.TRAJECTORY_HUBER, float(config.REPAIR_MAX_GAP)]))
    assert not (run["trajectory_status"] == 4).any() and (run["trajectory_cost"][:, 1] <= run["trajectory_cost"][:, 0]).all()
    outside = run["trajectory_status"] == 0
    assert np.array_equal(run["points3d_trajectory"][outside], plain["points3d_wo_procrustes"][outside])
    # what the method returns, and what the oracle says from the same start
    r = core.trajectory_triangulation()
    assert isinstance(r, ops.TrajectoryResult) and len(fits) == 2
    for key, value in zip(Core._TRAJECTORY_KEYS[:7], (r.points3d, r.status, r.weight, r.error, r.iterations, r.cost, r.counts)):
        assert isinstance(value, np.ndarray) and _same_value(run[key], value), key
    px = np.ascontiguousarray(core.camNet.points2d, dtype=np.float64)
    P = np.stack([c.P for c in core.camNet.cam_list])
    r64, _, moved, bar = _reference(P, px, plain["points3d_wo_procrustes"])
    assert (r64["fit_status"] == to.CONVERGED).all() and np.array_equal(r.status, r64["status"]) and np.array_equal(r.counts, r64["counts"])
    print(f"the golden recording: |device - oracle| {np.abs(r.points3d - r64['X']).max():.2e}, bar {bar:.2e}, status counts "
          f"{r.counts.sum(axis=0).tolist()}, iterations at most {r.iterations.max()}")
    assert np.abs(r.points3d - r64["X"]).max() <= bar
    # robust -> trajectory -> repair -> the angles, each stage once
    del fits[:], votes[:]
    core.save(joint_angles=True, repair_pose=True, robust_triangulation=True, robust_tau=2.0, trajectory_triangulation=True, trajectory_lambda=1e3)
    run = _load(pkl)
    assert list(run) == (list(plain) + ["joint_angles", "segment_lengths"] + list(Core._REPAIR_KEYS) + list(Core._ROBUST_KEYS)
                         + list(Core._TRAJECTORY_KEYS))
    assert all(_same_value(run[k], plain[k]) for k in plain) and fits == ["triangulate_trajectory"] and votes == ["triangulate_consensus"]
    robust = core.robust_triangulation(tau=2.0)
    assert _same_value(run["points3d_robust"], robust.points3d)
    kept = ((robust.cameras[None] >> np.arange(7)[:, None, None]) & 1).astype(bool) | (robust.status == 0)[None]
    assert (~kept & (px != 0.0).all(axis=-1)).any()                      # tau = 2 px rejects views of the golden recording
    want = ops.triangulate_trajectory(P, _dev(np.where(kept[..., None], px, 0.0), cuda), _dev(robust.points3d, cuda), lam=1e3)
    assert _same_value(run["points3d_trajectory"], want.points3d.cpu().numpy()) and _same_value(run["trajectory_weight"], want.weight.cpu().numpy())
    assert not run["trajectory_weight"][~kept].any()                      # a rejected view is no evidence
    assert run["trajectory_params"].tolist() == [1e3] * 38 + [config.TRAJECTORY_HUBER, float(config.REPAIR_MAX_GAP)]
    repaired = ops.repair_pose(want.points3d)
    assert _same_value(run["points3d_repaired"], repaired.points.cpu().numpy())
    assert np.array_equal(run["joint_angles"], ops.joint_angles(repaired.points)[0].cpu().numpy(), equal_nan=True)
    # without the repair the angles are the trajectory pose's own
    core.save(joint_angles=True, trajectory_triangulation=True)
    run = _load(pkl)
    assert list(run) == list(plain) + ["joint_angles", "segment_lengths"] + list(Core._TRAJECTORY_KEYS)
    angles = ops.joint_angles(_dev(run["points3d_trajectory"], cuda))[0].cpu().numpy()
    assert np.array_equal(run["joint_angles"], angles, equal_nan=True)
    core.save()
    assert _same_value(_load(pkl), plain)                                 # and the flag leaves nothing behind
    settings.pop("image_shape", None)


def test_cli_skip_pose_estimation_trajectory_triangulation(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config as settings
    from deepfly3d_amd.core import Core

    settings.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    order = [str(c) for c in range(7)]
    assert cli.main([folder, "--skip-pose-estimation", "--trajectory-triangulation", "--trajectory-lambda", "100", "--trajectory-huber", "5",
                     "--trajectory-max-gap", "2", "--order"] + order) == 0
    run = _load(pkl)
    assert list(run)[-8:] == list(Core._TRAJECTORY_KEYS) and run["trajectory_params"].tolist() == [100.0] * 38 + [5.0, 2.0]
    assert run["points3d_trajectory"].shape == run["points3d_wo_procrustes"].shape and run["trajectory_counts"].sum() == 15 * 38
    status = run["trajectory_status"]
    assert np.array_equal(run["trajectory_counts"], np.stack([(status == k).sum(axis=0) for k in range(5)], axis=1))
    settings.pop("image_shape", None)
