"""GPU tests of the pose repair against tests/pose_repair_oracle.py: flags, score, points, status and counts
are the oracle's, bit for bit (a NaN in the same place; its payload is not the model's), at every size where the kernels take another
path; the planted walker through ops.repair_pose and ops.gait; two bit-equal runs of the raw entries inside guard words; and Core and
the command line on the golden recording."""
import functools
import hashlib
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402
import pose_repair_oracle as pr  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = pr.TILE   # the outlier kernel's tile and the scan's block
REPAIR_KEYS = ["points3d_repaired", "repair_status", "repair_counts", "repair_score", "repair_params"]


def _sizes(h):
    # the clipped window (1, 2, h, h + 1, 2 h, 2 h + 1), a tile's edge, many tiles; at h = 2 more than 256 blocks per row: the scan's carry
    return sorted({1, 2, h, h + 1, 2 * h, 2 * h + 1, TILE - 1, TILE, TILE + 1, 2049} | ({65537} if h == 2 else set()))


CASES = [(h, T) for h in (1, 2, 5, 64) for T in _sizes(h)]


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the shared references are read-only


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _bits_where_finite(a, b):
    """NaN in the same places and the same bits everywhere else."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and _bits(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


def _same_repair(got, want):
    """got: (flags, score, points, status, counts) as numpy arrays, flags None where a caller does not return them; want: the oracle's
    dict."""
    flags, score, points, status, counts = got
    assert flags is None or (flags.dtype == np.uint8 and _bits(flags, want["flags"])), "flags"
    assert _bits_where_finite(score, want["score"]), "score"
    assert _bits_where_finite(points, want["points"]), "points"   # (a good joint is never NaN: the NaN of a missing one comes out as 0)
    assert status.dtype == np.int8 and _bits(status, want["status"]), "status"
    assert counts.dtype == np.int64 and _bits(counts, want["counts"]), "counts"


def _run(ops, Xd, **kw):
    flags, score = ops.pose_outliers(Xd, kw.get("half_window"), kw.get("threshold"), kw.get("floor"), kw.get("min_count"))
    points, status, counts = ops.fill_gaps(Xd, flags, kw.get("max_gap"))
    return tuple(a.cpu().numpy() for a in (flags, score, points, status, counts))


@functools.lru_cache(maxsize=None)
def _case(h, T):
    """(X, the oracle's repair of it with the default parameters but h): computed once and left unchanged."""
    X = pr.tied_poses(T, h, seed=1000 * h + T)
    want = pr.repair(X, h=h)
    for a in (X, *want.values()):
        a.setflags(write=False)
    return X, want


# ------------------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("h,T", CASES)
def test_repair_is_the_oracles(native_lib, cuda, h, T):
    """gait_oracle.random_poses with planted ties (a run of one value longer than the window, half of every window identical, steps
    of three frames), gaps across the edges of a tile and of a scan block, a joint that is good only in the last lane of a block and
    the first of the next, a joint missing throughout, NaN, infinity and signed zeros (pose_repair_oracle.tied_poses)."""
    from deepfly3d_amd import ops

    X, want = _case(h, T)
    got = _run(ops, _dev(X, cuda), half_window=h)
    _same_repair(got, want)
    r = ops.repair_pose(_dev(X, cuda), half_window=h)
    assert r.params == (h, pr.K, pr.FLOOR, pr.MAX_GAP, pr.N_MIN) and r.status.dtype == torch.int8
    assert _bits_where_finite(r.points.cpu().numpy(), want["points"]) and _bits(r.counts.cpu().numpy(), want["counts"])
    print(f"h = {h}, T = {T}: {int((want['flags'] & 2).astype(bool).sum())} outliers, codes {want['counts'].sum(axis=0).tolist()}")


@pytest.mark.parametrize("h", (1, 2, 5, 64))
def test_other_parameters(native_lib, cuda, h):
    """n_min = 1 and 2 h + 1, floor = 0 (ties give thr = 0: scores of 0 and +inf), thresholds other than the default, and max_gap = 0, 1
    and 1 000 000."""
    from deepfly3d_amd import ops

    T = 2 * TILE + 37
    X = pr.tied_poses(T, h, seed=h)
    Xd = _dev(X, cuda)
    for n_min, floor, k, gap in ((1, 0.0, 6.0, 0), (2 * h + 1, 0.05, 2.5, 1), (1, 0.0, 0.75, 1000000), (3, 1e-3, 6.0, 1000000)):
        want = pr.repair(X, h=h, k=k, floor=floor, max_gap=gap, n_min=n_min)
        _same_repair(_run(ops, Xd, half_window=h, threshold=k, floor=floor, min_count=n_min, max_gap=gap), want)
        if floor == 0.0:
            assert np.isinf(want["score"]).any() and (want["score"] == 0.0).any()
    # all joints missing; and nothing missing, nothing flagged
    gone = np.zeros((T, 38, 3))
    gone[::3] = np.nan
    got = _run(ops, _dev(gone, cuda), half_window=h)
    _same_repair(got, pr.repair(gone, h=h))
    assert np.all(got[3] == pr.MISSING_LEFT) and not got[2].any() and np.isnan(got[1]).all()
    calm = np.ones((T, 38, 3)) + np.arange(T)[:, None, None] * 1e-4
    got = _run(ops, _dev(calm, cuda), half_window=h)
    _same_repair(got, pr.repair(calm, h=h))
    assert not got[0].any() and _bits(got[2], calm) and got[4][:, 0].tolist() == [T] * 38


def test_gaps_across_block_edges(native_lib, cuda):
    """Hand-made flags: gaps that end on, start on and span the edges of the scan's blocks of 256, a gap of several blocks, gaps of
    exactly max_gap and max_gap + 1 frames, a joint whose only good frames are the first and the last."""
    from deepfly3d_amd import ops

    T = 5 * TILE + 3
    rng = np.random.default_rng(4)
    X = rng.normal(size=(T, 38, 3))
    flags = np.zeros((T, 38), dtype=np.uint8)
    flags[TILE - 4:TILE, 0] = 1            # ends on the edge
    flags[TILE:TILE + 4, 1] = 2            # starts on it
    flags[TILE - 2:TILE + 2, 2] = 1        # spans it
    flags[TILE - 1, 3] = flags[TILE, 3] = 2
    flags[10:3 * TILE + 10, 4] = 1         # several blocks
    flags[1:T - 1, 5] = 2                  # good in the first and the last frame alone
    flags[20:30, 6] = 1                    # exactly 10
    flags[20:31, 7] = 1                    # 11
    flags[:, 8] = 3
    flags[0, 9] = flags[T - 1, 9] = 2      # the ends
    flags[:, 10:] = (rng.random((T, 28)) < 0.4) * rng.integers(1, 4, (T, 28)).astype(np.uint8)
    Xd, fd = _dev(X, cuda), _dev(flags, cuda)
    for gap in (0, 1, 10, 11, 3 * TILE, 1000000):
        want = pr.fill_gaps(X, flags, gap)
        got = ops.fill_gaps(Xd, fd, gap)
        assert all(_bits(g.cpu().numpy(), w) for g, w in zip(got, want)), gap
    assert np.all(pr.fill_gaps(X, flags, 10)[1][20:30, 6] == pr.MISSING_FILLED) and np.all(pr.fill_gaps(X, flags, 10)[1][20:31, 7] == pr.MISSING_LEFT)
    assert np.all(pr.fill_gaps(X, flags, 1000000)[1][1:T - 1, 5] == pr.OUTLIER_FILLED)


# ------------------------------------------------------------------------------------------------------------------ the planted walker
@pytest.mark.parametrize("h", (2, 3, 5, 8))
def test_planted_spikes_and_the_gait(native_lib, cuda, golden_dir, h):
    from deepfly3d_amd import ops

    pose = go.planted_pose(golden_dir)
    X, placed = pr.planted_spikes(pr.noisy_walker(pose), h)
    r = ops.repair_pose(_dev(X, cuda), half_window=h)
    want = pr.repair(X, h=h)
    assert _bits_where_finite(r.points.cpu().numpy(), want["points"]) and _bits(r.status.cpu().numpy(), want["status"])
    assert _bits_where_finite(r.score.cpu().numpy(), want["score"])
    spikes = np.zeros((len(X), 38), dtype=bool)
    spikes[tuple(np.array(placed).T)] = True
    status = r.status.cpu().numpy()
    assert np.array_equal(status == pr.OUTLIER_FILLED, spikes) and (status == pr.MISSING_FILLED).sum() == 2 and not (status >= 3).any()
    g = ops.gait(r.points, go.PLANTED["fps"])
    planted = go.planted_lift_offs()
    steps = [(leg, t0, t2) for leg in range(6) for t0, t2 in zip(planted[leg][:-1], planted[leg][1:])]
    assert len(steps) == 171 and [(leg, t0, t2) for leg, t0, _, t2 in g.steps.cpu().numpy().tolist()] == steps
    assert ops.gait(_dev(X, cuda), go.PLANTED["fps"]).steps.cpu().numpy()[:, [0, 1, 3]].tolist() != [list(s) for s in steps]


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_determinism_guard_words_and_a_side_stream(native_lib, cuda):
    """The raw entries on poisoned buffers inside guard words, the workspace too, on a stream of their own: two runs are bit-equal,
    every output element is written and nothing outside is.  A null score changes nothing else."""
    lib = native_lib
    T, h = 9 * TILE + 41, 5
    X = pr.tied_poses(T, h, seed=77)
    want = pr.repair(X, h=h, k=4.0, floor=0.01, max_gap=6, n_min=2)
    GUARD = 64
    need = lib.df3d_repair_work_bytes(T)
    assert need % 16 == 0
    side = torch.cuda.Stream(device=cuda)
    st = side.cuda_stream
    fills = {torch.float64: -1.2345e30, torch.uint8: 0xEE, torch.int8: -77, torch.int64: -7777}

    def guarded(count, dtype=torch.float64):
        t = torch.full((count + 2 * GUARD,), fills[dtype], dtype=dtype, device=cuda)
        return t, t.data_ptr() + GUARD * t.element_size()

    def inner(t):
        a = t.cpu().numpy()
        fill = a.dtype.type(fills[t.dtype])
        assert np.all(a[:GUARD] == fill) and np.all(a[-GUARD:] == fill), "a guard word was written"
        return a[GUARD:-GUARD]

    runs = []
    with torch.cuda.stream(side):
        Xd = _dev(X, cuda)
        for with_score in (True, True, False):
            flags, score = guarded(T * 38, torch.uint8), guarded(T * 38)
            out, status, counts = guarded(T * 114), guarded(T * 38, torch.int8), guarded(38 * 5, torch.int64)
            work = guarded(need // 8)
            for rc in (lib.df3d_repair_outliers(Xd.data_ptr(), T, h, 4.0 * 1.4826, 0.01, 2, flags[1], score[1] if with_score else None, st),
                       lib.df3d_repair_fill(Xd.data_ptr(), flags[1], T, 6, out[1], status[1], counts[1], work[1], need, st)):
                assert rc == 0, lib.df3d_last_error()
            side.synchronize()
            inner(work[0])
            runs.append({k: inner(v[0]).copy() for k, v in dict(flags=flags, score=score, out=out, status=status, counts=counts).items()})
    first, second, blind = runs
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), f"{k} differs between two runs"
        if k != "score":
            assert first[k].tobytes() == blind[k].tobytes(), f"{k} depends on the score being asked for"
        if k in ("score", "out"):
            assert not np.any(first[k] == fills[torch.float64]), f"{k} was not written everywhere"
    assert np.all(blind["score"] == fills[torch.float64])   # a null score: nothing written
    _same_repair((first["flags"].reshape(T, 38), first["score"].reshape(T, 38), first["out"].reshape(T, 38, 3), first["status"].reshape(T, 38),
                  first["counts"].reshape(38, 5)), want)   # equal to the oracle: no poison is left in the integer outputs either


# ------------------------------------------------------------------------------------------------------------------ ops
def test_non_contiguous_and_empty_input(native_lib, cuda):
    from deepfly3d_amd import ops

    T = 300
    X = pr.tied_poses(T, 5, seed=5)
    plain = ops.repair_pose(_dev(X, cuda))
    wide = _dev(np.repeat(X, 2, axis=2), cuda)[:, :, ::2]   # not contiguous: ops copies
    assert not wide.is_contiguous()
    again = ops.repair_pose(wide)
    for name in ("points", "status", "counts", "score"):
        assert _bits_where_finite(getattr(plain, name).cpu().numpy().astype(np.float64), getattr(again, name).cpu().numpy().astype(np.float64)), name
    flags, _ = ops.pose_outliers(_dev(X, cuda))
    flags2 = torch.stack((flags, flags), dim=2)[:, :, 1]
    assert not flags2.is_contiguous()
    assert all(torch.equal(a, b) for a, b in zip(ops.fill_gaps(wide, flags2), (plain.points, plain.status, plain.counts)))
    empty = ops.repair_pose(torch.zeros((0, 38, 3), dtype=torch.float64, device=cuda))
    assert empty.points.shape == (0, 38, 3) and empty.status.shape == (0, 38) and empty.status.dtype == torch.int8 and empty.score.shape == (0, 38)
    assert empty.counts.shape == (38, 5) and empty.counts.dtype == torch.int64 and not empty.counts.any() and empty.params == (5, 6.0, 0.05, 10, 3)
    flags, score = ops.pose_outliers(torch.zeros((0, 38, 3), dtype=torch.float64, device=cuda))
    assert flags.shape == (0, 38) and flags.dtype == torch.uint8 and score.shape == (0, 38)
    with pytest.raises(ValueError, match=r"flags must be a torch.uint8 tensor of shape \[300, 38\]"):
        ops.fill_gaps(_dev(X, cuda), flags)
    with pytest.raises(ValueError, match="flags must be a torch.uint8 tensor"):
        ops.fill_gaps(_dev(X, cuda), torch.zeros((T, 38), dtype=torch.int32, device=cuda))


def test_pose_chain_repaired(native_lib, cuda):
    from deepfly3d_amd import ops
    from deepfly3d_amd.kinematics import PoseChain

    X = go.random_poses(200, seed=8)   # (every leg joint is seen in some frame: the fit needs a length for every segment)
    X[50, 7, 2] += 3.0
    chain = PoseChain(_dev(X, cuda), 100.0)
    fixed = chain.repaired(max_gap=4)
    want = ops.repair_pose(_dev(X, cuda), max_gap=4)
    host = lambda t: t.cpu().numpy()   # noqa: E731
    assert fixed.repair.params == (5, 6.0, 0.05, 4, 3) and _bits(host(fixed.points3d), host(want.points)) and fixed.fps == 100.0 and chain.repair is None
    assert fixed.measured is None and _bits(host(fixed.frame), host(ops.recording_frame(want.points)))   # a recording frame of its own
    rigid = fixed.rigid()
    assert rigid.measured is fixed and _bits_where_finite(host(rigid.points3d), host(ops.fit_legs(want.points).points))   # the fit of the repaired pose
    with pytest.raises(ValueError, match="half_window must be"):
        chain.repaired(half_window=0)


# ------------------------------------------------------------------------------------------------------------------ Core, command line
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


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_core_repair_pose(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    r = core.repair_pose()
    assert isinstance(r, ops.PoseRepairResult) and all(isinstance(a, np.ndarray) for a in (r.points, r.status, r.counts, r.score))
    assert r.params == (cfg.REPAIR_HALF_WINDOW, cfg.REPAIR_THRESHOLD, cfg.REPAIR_FLOOR, cfg.REPAIR_MAX_GAP, cfg.REPAIR_MIN_COUNT)
    X = np.ascontiguousarray(core.camNet.points3d, dtype=np.float64)
    want = pr.repair(X)
    _same_repair((None, r.score, r.points, r.status, r.counts), want)
    assert r.counts.sum() == 15 * 38
    print(f"the golden recording: codes {r.counts.sum(axis=0).tolist()}")
    other = core.repair_pose(half_window=2, threshold=3.0, floor=0.0, max_gap=1, min_count=2)
    assert other.params == (2, 3.0, 0.0, 1, 2)
    want = pr.repair(X, h=2, k=3.0, floor=0.0, max_gap=1, n_min=2)
    _same_repair((None, other.score, other.points, other.status, other.counts), want)
    # the other methods of the repaired pose: ops on the repaired array
    fixed = _dev(r.points, cuda)
    g, mine = core.gait(repair=True), ops.gait(fixed, cfg.SPECTROGRAM_FPS)
    for name in ("tip", "vel", "states", "steps", "step_metrics", "phase", "pattern"):
        assert _bits_where_finite(getattr(g, name).astype(np.float64), getattr(mine, name).cpu().numpy().astype(np.float64)), name
    angles, lengths = core.joint_angles(repair=True, rigid=True)
    fit = ops.fit_legs(fixed)
    want_angles, want_lengths = ops.joint_angles(fit.points, ops.recording_frame(fixed))   # the repaired pose's own recording frame
    assert _bits_where_finite(angles, want_angles.cpu().numpy()) and _bits_where_finite(lengths, want_lengths.cpu().numpy())
    assert _bits_where_finite(core.rigid_legs(repair=True)[0], fit.points.cpu().numpy())
    plain = core.joint_angles()
    assert _bits_where_finite(core.joint_angles(repair=False)[0], plain[0])
    assert _bits_where_finite(core.joint_angles(repair=True)[0], ops.joint_angles(fixed)[0].cpu().numpy())
    # a save without the flag writes what the code before this stage wrote: the digests tests/test_gpu_pose_chain.py pins
    with open(os.path.join(golden_dir, "pose_chain_save_digests.json")) as f:
        pinned = json.load(f)
    core.save(joint_angles=True, rigid_legs=True)
    run = _load(pkl)
    keys = ["joint_angles", "segment_lengths", "points3d_rigid", "rigid_segment_lengths", "rigid_fit_cost", "joint_angles_rigid"]
    assert list(run.keys())[-6:] == keys and {k: _digest(run[k]) for k in keys} == {k: pinned[k] for k in keys}
    with pytest.raises(ValueError, match="they need repair_pose=True"):
        core.save(repair_max_gap=3)
    config.pop("image_shape", None)


def _digest(v):
    h = hashlib.sha256()
    h.update(str(v.dtype).encode() + b"|" + repr(tuple(v.shape)).encode() + b"|" + np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def test_cli_skip_pose_estimation_repair_pose(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    from deepfly3d_amd import cli, ops
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    with open(pkl, "rb") as f:
        earlier = f.read()
    order = [str(c) for c in range(7)]
    calls = dict.fromkeys(("repair_pose", "fit_legs", "recording_frame"), 0)

    def counted(name, fn):
        def wrapper(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)

        return wrapper

    for name in calls:
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))

    def reopen(*flags):
        with open(pkl, "wb") as f:
            f.write(earlier)
        for name in calls:
            calls[name] = 0
        assert cli.main([folder, "--skip-pose-estimation", *flags, "--order"] + order) == 0
        return _load(pkl)

    plain = reopen("--joint-angles")
    fixed_keys = [k for k in plain if k not in ("joint_angles", "segment_lengths")]   # the keys that do not depend on the kinematics
    assert not [k for k in plain if str(k).startswith("repair") or k == "points3d_repaired"] and calls["repair_pose"] == 0   # without the flag
    for others in (("--joint-angles", "--gait"), ("--joint-angles", "--gait", "--rigid-legs")):
        before = reopen(*others)
        run = reopen(*others, "--repair-pose")
        assert calls["repair_pose"] == 1 and calls["recording_frame"] == 1 and calls["fit_legs"] == (1 if "--rigid-legs" in others else 0)   # once per save
        assert list(run.keys()) == list(before.keys()) + REPAIR_KEYS   # after every existing key
        assert all(_same(before[k], run[k]) for k in fixed_keys)       # the triangulation's own keys, byte for byte
        want = pr.repair(run["points3d_wo_procrustes"])
        assert run["repair_status"].dtype == np.int8 and run["repair_counts"].shape == (38, 5)
        _same_repair((None, run["repair_score"], run["points3d_repaired"], run["repair_status"], run["repair_counts"]), want)
        assert run["repair_params"].dtype == np.float64 and run["repair_params"].tolist() == [5.0, 6.0, 0.05, 10.0, 3.0]
        fixed = _dev(run["points3d_repaired"], cuda)
        angles, lengths = ops.joint_angles(fixed)
        assert _bits_where_finite(run["joint_angles"], angles.cpu().numpy()) and _bits_where_finite(run["segment_lengths"], lengths.cpu().numpy())
        assert _bits_where_finite(run["gait_tip_velocity"], ops.gait(fixed, run["gait_fps"]).vel.cpu().numpy())
        if "--rigid-legs" in others:
            assert _bits_where_finite(run["points3d_rigid"], ops.fit_legs(fixed).points.cpu().numpy())
    alone = reopen("--repair-pose", "--repair-window", "2", "--repair-threshold", "3", "--repair-floor", "0", "--repair-max-gap", "1")
    assert list(alone.keys()) == fixed_keys + REPAIR_KEYS and alone["repair_params"].tolist() == [2.0, 3.0, 0.0, 1.0, 3.0] and calls["repair_pose"] == 1
    want = pr.repair(alone["points3d_wo_procrustes"], h=2, k=3.0, floor=0.0, max_gap=1)
    _same_repair((None, alone["repair_score"], alone["points3d_repaired"], alone["repair_status"], alone["repair_counts"]), want)
    with open(pkl, "wb") as f:
        f.write(earlier)
    with pytest.raises(SystemExit):
        cli.main([folder, "--skip-pose-estimation", "--repair-max-gap", "3", "--order"] + order)
    with open(pkl, "rb") as f:
        assert f.read() == earlier   # refused before any work: the earlier result is untouched
    config.pop("image_shape", None)
