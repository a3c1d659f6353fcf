"""GPU tests of the leg joint angles: ops.joint_angles / ops.body_frame (df3d_joint_angles, df3d_body_frame)
against the float64 oracle tests/joint_angles_oracle.py on the golden recording, on forward-kinematics flies (also against the
angles they were built from), over the sizes that cross a wave, a block and a partial last block, with explicit frames, on exactly
degenerate integer poses, under rigid motions; buffers and the NULL lengths pointer; Core.joint_angles and --joint-angles.

Bars.  Angles: 1e-10 rad after wrapping the difference to (-pi, pi]; lengths: 1e-12 relative; NaN positions identical; nothing is
excluded.  The angle bar is derived, not measured: every input here keeps each sine that enters a tors() or thc_pitch at or above
0.05 (asserted through jo.min_sine) or makes it exactly zero, so the arguments of atan2 carry at most a few tens of ulp / 0.05^2 ~ 1e-12 of relative error with or without fused multiply-adds; 1e-10 leaves two orders of margin and is smooth.hip's bar."""
import os
import pickle

import numpy as np
import pytest
import torch

import joint_angles_oracle as jo

pytestmark = pytest.mark.gpu

ANGLE_TOL, LENGTH_RTOL, BUILT_TOL, MIN_SINE = 1e-10, 1e-12, 1e-9, 0.05


def _dev(cuda, a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(cuda)   # a copy: the shared fixtures are read-only


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _compare(got, want, what=""):
    (ga, gl), (wa, wl) = [tuple(_host(a) for a in x) for x in (got, want)]
    assert ga.shape == wa.shape and gl.shape == wl.shape
    assert np.array_equal(np.isnan(ga), np.isnan(wa)) and np.array_equal(np.isnan(gl), np.isnan(wl)), what
    assert not np.isinf(ga).any() and not np.isinf(gl).any()
    keep = ~np.isnan(wa)
    da = np.abs(jo.wrap(ga[keep] - wa[keep])).max() if keep.any() else 0.0
    keep = ~np.isnan(wl)
    dl = (np.abs(gl[keep] - wl[keep]) / np.maximum(wl[keep], 1e-300)).max() if keep.any() else 0.0
    print(f"{what}: angles off by {da:.3e} rad, lengths by {dl:.3e} relative")
    assert da <= ANGLE_TOL and dl <= LENGTH_RTOL, what


@pytest.fixture(scope="module")
def fk():
    """The 200 forward-kinematics flies, rotated, scaled by 1.7 and translated: (Y, the angles and lengths they were built from,
    R whose columns are the body axes), and the oracle's per-frame answer on them, computed once."""
    X, A, L = jo.random_fly(np.random.default_rng(14), 200)
    R = jo.random_rotation(np.random.default_rng(1))
    Y = 1.7 * X @ R.T + np.array([3.0, -2.0, 5.0])
    want = jo.joint_angles(Y, "per_frame")
    assert jo.min_sine(Y, "per_frame") >= MIN_SINE
    for a in (Y, A, L, R) + want:
        a.setflags(write=False)
    return Y, A, 1.7 * L, R, want


# ------------------------------------------------------------------------------------------------------------------ golden, forward kinematics
@pytest.mark.parametrize("key", ["points3d", "points3d_wo_procrustes"])
@pytest.mark.parametrize("mode", ["recording", "per_frame"])
def test_golden_recording_matches_the_oracle(native_lib, cuda, golden_dir, key, mode):
    from deepfly3d_amd import ops

    X = np.load(f"{golden_dir}/golden_3d.npz")[key]
    assert jo.min_sine(X, mode) >= MIN_SINE
    got = ops.joint_angles(_dev(cuda, X), mode)
    assert tuple(got[0].shape) == (15, 6, 8) and tuple(got[1].shape) == (15, 6, 4) and got[0].device == cuda
    _compare(got, jo.joint_angles(X, mode), f"golden {key} {mode}")
    frames = ops.body_frame(_dev(cuda, X))
    assert np.abs(_host(frames) - jo.body_frames(X)).max() < 1e-13


def test_forward_kinematics_flies_give_back_their_angles(native_lib, cuda, fk):
    from deepfly3d_amd import ops

    Y, A, L, R, want = fk
    got = ops.joint_angles(_dev(cuda, Y), "per_frame")
    _compare(got, want, "forward kinematics")
    ga, gl = _host(got[0]), _host(got[1])
    built = np.abs(jo.wrap(ga - A)).max()
    print(f"against the angles they were built from: {built:.3e} rad")
    assert built <= BUILT_TOL and np.abs(gl / L - 1.0).max() <= BUILT_TOL
    assert np.abs(_host(ops.body_frame(_dev(cuda, Y))) - R.T[None]).max() < 1e-12
    assert jo.min_sine(Y, "recording") >= MIN_SINE
    _compare(ops.joint_angles(_dev(cuda, Y)), jo.joint_angles(Y, "recording"), "forward kinematics, the recording's frame")


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_sizes_across_wave_and_block_boundaries(native_lib, cuda, fk, T):
    from deepfly3d_amd import ops

    Y, _, _, _, per_frame = fk
    idx = np.arange(T) % len(Y)
    Z = np.ascontiguousarray(Y[idx])
    Zd = _dev(cuda, Z)
    _compare(ops.joint_angles(Zd, "per_frame"), (per_frame[0][idx], per_frame[1][idx]), f"T = {T}, one frame per pose")   # nframes = T
    assert jo.min_sine(Z, "recording") >= MIN_SINE
    _compare(ops.joint_angles(Zd, "recording"), jo.joint_angles(Z, "recording"), f"T = {T}, one frame")   # nframes = 1


def test_explicit_frames(native_lib, cuda, fk):
    from deepfly3d_amd import ops

    Y = fk[0][:40]
    rng = np.random.default_rng(100)
    one = jo.random_rotation(rng)
    each = np.stack([jo.random_rotation(rng) for _ in range(len(Y))])
    Yd = _dev(cuda, Y)
    for F, given in ((one, one), (one, _dev(cuda, one)), (each, each), (each, _dev(cuda, each)), (one, one[None])):
        assert jo.min_sine(Y, F) >= MIN_SINE
        _compare(ops.joint_angles(Yd, given), jo.joint_angles(Y, F), f"explicit frame {np.shape(F)}")
    for bad in (np.eye(4), np.zeros((2, 3, 3)), np.zeros((3,))):
        with pytest.raises(ValueError):
            ops.joint_angles(Yd, bad)
    with pytest.raises(ValueError):
        ops.joint_angles(Yd, "thorax")
    # a frame that holds a NaN is used as given: its poses' angles are NaN, the lengths are not
    each = each.copy()
    each[7, 1, 2] = np.nan
    a, l = ops.joint_angles(Yd, each)
    assert torch.isnan(a[7]).all() and not torch.isnan(a[:7]).any() and not torch.isnan(a[8:]).any() and not torch.isnan(l).any()
    _compare((a, l), jo.joint_angles(Y, each), "a NaN frame")
    # no poses
    a, l = ops.joint_angles(Yd[:0])
    assert tuple(a.shape) == (0, 6, 8) and tuple(l.shape) == (0, 6, 4) and tuple(ops.body_frame(Yd[:0]).shape) == (0, 3, 3)


# ------------------------------------------------------------------------------------------------------------------ exact degenerates
SEG = np.array([[1, 2, -2], [2, 1, -3], [-1, 2, -2], [1, 1, -2]], dtype=np.float64)   # coxa, femur, tibia, tarsus in leg coordinates


def _integer_fly(segments=None):
    """[38, 3] small integers: under the identity frame every product the model forms is exact, with or without fused
    multiply-adds.  `segments` {leg: [4, 3]} replaces the segment vectors (leg coordinates) of the legs it names."""
    X = np.array([[j % 5 + 1, j % 3 + 2, j % 7 + 1] for j in range(38)], dtype=np.float64)   # antenna, stripes: anywhere but the origin
    for leg in range(6):
        side, l = divmod(leg, 3)
        mirror = np.array([1.0, -1.0 if side else 1.0, 1.0])
        seg = (SEG + np.array([l, 0, side])) if segments is None or leg not in segments else np.asarray(segments[leg], dtype=np.float64)
        P = np.array([4.0 - 3 * l, 2.0 + l, 1.0 + l]) * mirror
        for k, j in enumerate(jo.leg_joints(leg)):
            X[j] = P
            if k < 4:
                P = P + seg[k] * mirror
    assert not (X == 0).all(axis=1).any()
    return X


def _degenerate_cases():
    """[(name, pose [38, 3], the leg it touches)]: the integer fly with one defect each."""
    cases = []
    nan, inf = np.nan, np.inf
    # a missing joint at each of the five positions: zeros, a NaN, an infinity
    for k in range(5):
        for leg, (tag, value) in zip((k % 6, (k + 2) % 6, (k + 4) % 6), (("zeros", [0, 0, 0]), ("NaN", [1, nan, 2]), ("inf", [-inf, 3, 1]))):
            X = _integer_fly()
            X[jo.leg_joints(leg)[k]] = value
            cases.append((f"joint {k} missing ({tag})", X, leg))
    base = SEG.copy()
    for leg in (0, 4):
        s = base.copy()
        s[1] = 0                                     # coxa-femur and femur-tibia joints coincide: a femur of length 0
        cases.append(("coincident joints", _integer_fly({leg: s}), leg))
        s = base.copy()
        s[1] = 2 * s[0]                              # straight coxa-femur
        cases.append(("straight coxa-femur", _integer_fly({leg: s}), leg))
        s = base.copy()
        s[2] = s[1]                                  # straight femur-tibia
        cases.append(("straight femur-tibia", _integer_fly({leg: s}), leg))
        s = base.copy()
        s[3] = 3 * s[2]                              # straight tibia-tarsus
        cases.append(("straight tibia-tarsus", _integer_fly({leg: s}), leg))
        for sign in (1, -1):
            s = base.copy()
            s[0] = [0, 3 * sign, 0]                  # the coxa along +-y (outward / inward)
            cases.append((f"coxa along {'+' if sign > 0 else '-'}y", _integer_fly({leg: s}), leg))
    return cases


def test_exact_degenerate_cases(native_lib, cuda):
    from deepfly3d_amd import ops

    cases = _degenerate_cases()
    base = _integer_fly()
    X = np.stack([base] + [c[1] for c in cases])
    F = np.eye(3)
    assert jo.min_sine(base[None], F) >= MIN_SINE
    want = jo.joint_angles(X, F)
    got = tuple(_host(t) for t in ops.joint_angles(_dev(cuda, X), F))
    _compare(got, want, "exact degenerates")
    ga, gl = got
    assert not np.isnan(ga[0]).any() and not np.isnan(gl[0]).any()
    isnan = lambda row: [bool(v) for v in np.isnan(row)]   # noqa: E731
    for i, (name, _, leg) in enumerate(cases, start=1):
        others = [x for x in range(6) if x != leg]
        assert np.array_equal(ga[i, others], ga[0, others]) and np.array_equal(gl[i, others], gl[0, others]), name   # untouched legs
        a, l = ga[i, leg], gl[i, leg]
        if name.startswith("joint"):
            k = int(name.split()[1])
            gone = [s for s in range(4) if s in (k - 1, k)]   # the segments that end at joint k
            assert isnan(l) == [s in gone for s in range(4)], name
            uses = [[0], [0], [0, 1], [0, 1], [0, 1, 2], [1, 2], [1, 2, 3], [2, 3]]
            assert isnan(a) == [bool(set(u) & set(gone)) for u in uses], name
        elif name == "coincident joints":
            assert l[1] == 0.0 and isnan(l) == [False] * 4 and isnan(a) == [False, False, True, True, True, True, True, False], name
        elif name == "straight coxa-femur":
            assert a[3] == 0.0 and isnan(a) == [False, False, True, False, True, False, False, False], name
        elif name == "straight femur-tibia":
            assert a[5] == 0.0 and isnan(a) == [False, False, False, False, True, False, True, False], name
        elif name == "straight tibia-tarsus":
            assert a[7] == 0.0 and isnan(a) == [False, False, False, False, False, False, True, False], name
        else:
            sign = 1.0 if "+" in name else -1.0
            assert abs(a[0] - sign * np.pi / 2) < 1e-15 and isnan(a) == [False, True, True, False, False, False, False, False], name


def test_missing_body_coxa_joint_blanks_its_own_pose_only(native_lib, cuda, fk):
    from deepfly3d_amd import ops

    Y = fk[0][:12].copy()
    clean = ops.joint_angles(_dev(cuda, Y), "per_frame")
    Y[3, 24] = 0.0                       # side 1's mid body-coxa joint
    Y[9, 0, 1] = np.inf                  # side 0's front one
    got = ops.joint_angles(_dev(cuda, Y), "per_frame")
    _compare(got, jo.joint_angles(Y, "per_frame"), "a missing body-coxa joint")
    a, l = got
    assert torch.isnan(a[[3, 9]]).all()
    rest = [t for t in range(12) if t not in (3, 9)]
    assert torch.equal(a[rest], clean[0][rest]) and torch.equal(l[rest], clean[1][rest])
    assert torch.isnan(l[3, 4, 0]) and torch.isnan(l[9, 0, 0]) and int(torch.isnan(l).sum()) == 2   # the two coxae that end there
    frames = ops.body_frame(_dev(cuda, Y))
    assert torch.isnan(frames[[3, 9]]).all() and not torch.isnan(frames[rest]).any()
    # coincident sides: no left-right axis
    Z = fk[0][:2].copy()
    Z[1, 19:] = Z[1, :19]
    frames = ops.body_frame(_dev(cuda, Z))
    assert torch.isnan(frames[1]).all() and not torch.isnan(frames[0]).any()
    assert np.isnan(jo.body_frame(Z[1])).all()


# ------------------------------------------------------------------------------------------------------------------ equivariance, buffers
def test_rigid_motion_and_scale_on_the_device(native_lib, cuda, fk):
    from deepfly3d_amd import ops

    Y = fk[0][:64]
    rng = np.random.default_rng(5)
    a0, l0 = (_host(t) for t in ops.joint_angles(_dev(cuda, Y), "per_frame"))
    for scale in (1.0, 0.013, 250.0):
        Z = scale * Y @ jo.random_rotation(rng).T + rng.normal(0, 3, 3) * scale
        assert jo.min_sine(Z, "per_frame") >= MIN_SINE
        a, l = (_host(t) for t in ops.joint_angles(_dev(cuda, Z), "per_frame"))
        da, dl = np.abs(jo.wrap(a - a0)).max(), np.abs(l / (scale * l0) - 1.0).max()
        print(f"scale {scale}: angles move by {da:.3e} rad, lengths by {dl:.3e} relative")
        # the moved points are rounded once more: 1.1e-16 of coordinates up to ~30 segment lengths, a few 1e-15 of a segment's length
        # and direction, which the sines >= 0.05 amplify to ~1e-12 rad at the most: inside the two bars
        assert da < ANGLE_TOL and dl <= LENGTH_RTOL


def test_outputs_are_written_fully_and_lengths_may_be_null(native_lib, cuda, fk):
    Y, _, _, _, want = fk
    sentinel = -12345.678
    for T in (1, 65, 200):
        Yd = _dev(cuda, Y[:T])
        frames = torch.empty((T, 3, 3), dtype=torch.float64, device=cuda).fill_(sentinel)
        assert native_lib.df3d_body_frame(Yd.data_ptr(), T, frames.data_ptr(), None) == 0
        for with_lengths in (True, False):
            guard = 16   # doubles past the end: must stay untouched
            ang = torch.full((T * 48 + guard,), sentinel, dtype=torch.float64, device=cuda)
            length = torch.full((T * 24 + guard,), sentinel, dtype=torch.float64, device=cuda)
            rc = native_lib.df3d_joint_angles(Yd.data_ptr(), T, frames.data_ptr(), T, ang.data_ptr(), length.data_ptr() if with_lengths else None, None)
            assert rc == 0, native_lib.df3d_last_error()
            torch.cuda.synchronize()
            assert not (frames == sentinel).any() and not (ang[: T * 48] == sentinel).any() and (ang[T * 48:] == sentinel).all()
            if with_lengths:
                assert not (length[: T * 24] == sentinel).any() and (length[T * 24:] == sentinel).all()
                _compare((ang[: T * 48].view(T, 6, 8), length[: T * 24].view(T, 6, 4)), (want[0][:T], want[1][:T]), f"ctypes, T = {T}")
            else:
                assert (length == sentinel).all()
                _compare((ang[: T * 48].view(T, 6, 8), want[1][:T]), (want[0][:T], want[1][:T]), f"ctypes without lengths, T = {T}")


# ------------------------------------------------------------------------------------------------------------------ Core and the CLI
def _recording(tmp_path, golden_dir, with_cameras):
    """(folder, result pickle): 15 frames (links to the sample's frame 0) and an earlier result holding the golden detections and,
    `with_cameras`, the golden cameras."""
    folder = tmp_path / "working"
    folder.mkdir()
    for c in range(7):
        for t in range(15):
            os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
    folder = str(folder)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    os.makedirs(folder + "_df3d")
    pkl = os.path.join(folder + "_df3d", "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
    res = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "distort": g3["distort"][c], "intr": g3["intr"][c]} for c in range(7)} if with_cameras else {}
    res.update(points2d=g3["points2d"], camera_ordering=g3["camera_ordering"], heatmap_confidence=g3["heatmap_confidence"])
    with open(pkl, "wb") as f:
        pickle.dump(res, f)
    return folder, pkl


def _load(pkl):
    with open(pkl, "rb") as f:
        return pickle.load(f)


def test_core_and_cli_end_to_end(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli, ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    folder, pkl = _recording(tmp_path, golden_dir, with_cameras=True)
    order = [str(c) for c in range(7)]
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    assert core.has_calibration and core.camNet.points3d is None
    angles, lengths = core.joint_angles()   # triangulates first
    assert isinstance(angles, np.ndarray) and angles.shape == (15, 6, 8) and lengths.shape == (15, 6, 4) and not np.isnan(angles).any()
    core.save()
    saved = _load(pkl)
    assert "joint_angles" not in saved and "segment_lengths" not in saved
    X = saved["points3d_wo_procrustes"]
    for mode in ("recording", "per_frame"):
        want = ops.joint_angles(_dev(cuda, X), mode)
        got = core.joint_angles(mode)
        assert np.array_equal(got[0], _host(want[0])) and np.array_equal(got[1], _host(want[1]))
        _compare(got, jo.joint_angles(X, mode), f"Core.joint_angles {mode}")
    plain_keys = list(saved.keys())
    core.save(joint_angles=True)
    flagged = _load(pkl)
    assert list(flagged.keys()) == plain_keys + ["joint_angles", "segment_lengths"]
    assert np.array_equal(flagged["joint_angles"], angles) and np.array_equal(flagged["segment_lengths"], lengths)
    # df3d-cli --skip-pose-estimation --joint-angles on the reopened result: calibrate_calc -> save, the two keys last
    assert cli.main([folder, "--skip-pose-estimation", "--joint-angles", "--order"] + order) == 0
    run = _load(pkl)
    assert [str(k) for k in run.keys()] == [str(k) for k in g3["key_order"]] + ["joint_angles", "segment_lengths"]
    want = ops.joint_angles(_dev(cuda, run["points3d_wo_procrustes"]))
    assert np.array_equal(run["joint_angles"], _host(want[0])) and np.array_equal(run["segment_lengths"], _host(want[1]))
    _compare((run["joint_angles"], run["segment_lengths"]), jo.joint_angles(run["points3d_wo_procrustes"]), "--joint-angles")
    # the same steps without the flag: neither key, everything else as in the flagged run
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    core.calibrate_calc(0, core.max_img_id)
    core.save()
    plain = _load(pkl)
    assert [str(k) for k in plain.keys()] == [str(k) for k in g3["key_order"]]
    for k in ("points2d", "heatmap_confidence", "camera_ordering"):
        assert np.array_equal(plain[k], run[k]), k
    for k in ("points3d_wo_procrustes", "points3d"):
        assert np.allclose(plain[k], run[k], atol=1e-9), k
    config.pop("image_shape", None)
