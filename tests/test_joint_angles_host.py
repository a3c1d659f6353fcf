"""CPU tests of the leg joint angles: the float64 oracle's own properties (forward-kinematics round trip,
mirror symmetry, the golden recording, axis permutations), the argument validation of df3d_body_frame / df3d_joint_angles (no
device is touched), the CLI flag, config's tables and Core.joint_angles' refusals."""
import ctypes
import itertools

import numpy as np
import pytest

import joint_angles_oracle as jo


@pytest.fixture(scope="module")
def fk():
    """(X, angles, lengths) of 200 forward-kinematics flies in the identity frame."""
    X, A, L = jo.random_fly(np.random.default_rng(14), 200)
    for a in (X, A, L):
        a.setflags(write=False)
    return X, A, L


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_forward_kinematics_round_trip(fk):
    X, A, L = fk
    rng = np.random.default_rng(1)
    R = jo.random_rotation(rng)
    Y = 1.7 * X @ R.T + np.array([3.0, -2.0, 5.0])
    assert np.abs(jo.body_frames(Y) - R.T[None]).max() < 1e-12   # rows ex, ey, ez: the rotated axes
    got, lengths = jo.joint_angles(Y, "per_frame")
    err = np.abs(jo.wrap(got - A)).max()
    print("round trip", err)
    assert not np.isnan(got).any() and err < 1e-12
    assert np.abs(lengths / (1.7 * L) - 1.0).max() < 1e-12


def test_mirror_image_has_the_same_angles(fk):
    X = fk[0][:40]
    rng = np.random.default_rng(2)
    Y = X @ jo.random_rotation(rng).T + rng.normal(size=3)   # a fly in general position
    M = np.concatenate([Y[:, 19:], Y[:, :19]], axis=1) * np.array([1.0, -1.0, 1.0])   # sides swapped, reflected in y = 0
    for mode in ("per_frame", "recording"):
        a, l = jo.joint_angles(Y, mode)
        am, lm = jo.joint_angles(M, mode)
        assert np.array_equal(am, a[:, [3, 4, 5, 0, 1, 2]]) and np.array_equal(lm, l[:, [3, 4, 5, 0, 1, 2]])


def test_golden_recording_is_far_from_every_degenerate_case(golden_dir):
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    for key in ("points3d", "points3d_wo_procrustes"):
        for mode in ("recording", "per_frame"):
            a, l = jo.joint_angles(g3[key], mode)
            assert a.shape == (15, 6, 8) and l.shape == (15, 6, 4)
            assert not np.isnan(a).any() and not np.isnan(l).any() and np.isfinite(a).all()
            assert jo.min_sine(g3[key], mode) >= 0.14
    # ez points away from the tarsus tips, on the recording's average
    X = g3["points3d_wo_procrustes"]
    F = jo.recording_frame(X)
    assert np.abs(F @ F.T - np.eye(3)).max() < 1e-15
    tips, coxae = X[:, [jo.leg_joints(leg)[4] for leg in range(6)]], X[:, jo.COXAE]
    assert ((tips - coxae).mean(axis=(0, 1)) @ F[2]) < -1.0


def _axis_rotations():
    """The 24 signed permutation matrices of determinant +1."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            Q = np.zeros((3, 3))
            Q[range(3), perm] = signs
            if np.linalg.det(Q) > 0:
                out.append(Q)
    assert len(out) == 24
    return out


def test_axis_rotations_leave_recording_mode_unchanged(fk, golden_dir):
    for X in (np.load(f"{golden_dir}/golden_3d.npz")["points3d_wo_procrustes"], fk[0][:15] + np.array([0.3, 0.1, -0.2])):
        a, l = jo.joint_angles(X, "recording")
        for Q in _axis_rotations():
            aq, lq = jo.joint_angles(X @ Q.T, "recording")
            assert np.abs(jo.wrap(aq - a)).max() < 1e-12 and np.abs(lq - l).max() < 1e-12


def test_oracle_nan_rules():
    X = jo.random_fly(np.random.default_rng(3), 2)[0]
    X[0, 7] = 0.0                 # leg 1's femur-tibia joint: femur and tibia go, the coxa stays
    X[1, 19] = np.nan             # a body-coxa joint: that pose's frame
    a, l = jo.joint_angles(X, "per_frame")
    assert np.isnan(a[1]).all() and np.isnan(l[1, 3, 0]) and not np.isnan(l[1, 3, 1:]).any() and not np.isnan(l[1, [0, 1, 2, 4, 5]]).any()
    assert not np.isnan(a[0, [0, 2, 3, 4, 5]]).any()
    assert np.array_equal(np.isnan(a[0, 1]), [False, False, True, True, True, True, True, True])
    assert np.array_equal(np.isnan(l[0, 1]), [False, True, True, False])


# ------------------------------------------------------------------------------------------------------------------ C entries
def test_entries_validate_arguments_without_gpu(native_lib):
    lib = native_lib
    assert hasattr(lib, "df3d_body_frame") and hasattr(lib, "df3d_joint_angles")
    base = 1 << 20
    pts, frame, ang, length = (ctypes.c_void_p(base + k * (1 << 16)) for k in range(4))   # T = 4: 3 648 + 72 + 1 536 + 768 bytes
    err = lib.df3d_last_error
    # no frames: nothing to do, whatever the pointers
    assert lib.df3d_joint_angles(None, 0, None, 1, None, None, None) == 0
    assert lib.df3d_body_frame(None, 0, None, None) == 0
    assert lib.df3d_joint_angles(pts, -1, frame, 1, ang, length, None) == -1 and b"T must be >= 0" in err()
    assert lib.df3d_body_frame(pts, -1, frame, None) == -1 and b"n must be >= 0" in err()
    for i in range(3):   # pts, frame, angles; lengths may be NULL
        args = [pts, frame, ang]
        args[i] = None
        assert lib.df3d_joint_angles(args[0], 4, args[1], 1, args[2], length, None) == -1 and b"null" in err(), i
    assert lib.df3d_body_frame(None, 4, frame, None) == -1 and b"null" in err()
    assert lib.df3d_body_frame(pts, 4, None, None) == -1 and b"null" in err()
    for nframes in (0, 2, 3, 5, -1):
        assert lib.df3d_joint_angles(pts, 4, frame, nframes, ang, length, None) == -1 and b"nframes" in err(), nframes
    # outputs that overlap the poses: at their first and their last byte, and the poses inside an output
    nbytes = 4 * 38 * 3 * 8
    for out in (base, base + nbytes - 16, base - 4 * 48 * 8 + 16):
        assert lib.df3d_joint_angles(pts, 4, frame, 1, ctypes.c_void_p(out), length, None) == -1 and b"overlap pts" in err(), out
        assert lib.df3d_joint_angles(pts, 4, frame, 1, ang, ctypes.c_void_p(out + 4 * 24 * 8 if out < base else out), None) == -1 and b"overlap pts" in err(), out
    assert lib.df3d_body_frame(pts, 4, ctypes.c_void_p(base + nbytes - 8), None) == -1 and b"overlap pts" in err()
    assert lib.df3d_body_frame(pts, 4, ctypes.c_void_p(base - 4 * 72 + 8), None) == -1 and b"overlap pts" in err()
    # ... the frames, or each other
    assert lib.df3d_joint_angles(pts, 4, frame, 4, ctypes.c_void_p(frame.value + 4 * 72 - 16), length, None) == -1 and b"overlap the frames" in err()
    assert lib.df3d_joint_angles(pts, 4, frame, 1, ang, ctypes.c_void_p(ang.value + 4 * 48 * 8 - 16), None) == -1 and b"each other" in err()
    assert lib.df3d_joint_angles(pts, 4, frame, 1, ctypes.c_void_p(ang.value + 8), length, None) == -1 and b"16-byte aligned" in err()


# ------------------------------------------------------------------------------------------------------------------ CLI, config, Core
def test_cli_joint_angles_flag_parses():
    from deepfly3d_amd.cli import parse_cli_args

    assert parse_cli_args(["/tmp/x", "--joint-angles"]).joint_angles is True
    assert parse_cli_args(["/tmp/x"]).joint_angles is False
    args = parse_cli_args(["/tmp/x", "--joint-angles", "--skip-pose-estimation"])   # on a reopened result
    assert args.joint_angles and args.skip_estimation


def test_cli_joint_angles_without_a_result_to_reopen_is_refused(tmp_path, golden_dir):
    import os

    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    config.pop("image_shape", None)
    args = cli.parse_cli_args([str(folder), "--joint-angles", "--skip-pose-estimation"])
    with pytest.raises(RuntimeError, match="--joint-angles needs calibrated cameras"):
        cli.run(args)
    config.pop("image_shape", None)
    assert not [f for f in os.listdir(str(folder) + "_df3d") if f.startswith("df3d_result")]


def test_config_leg_tables():
    from deepfly3d_amd import config as cfg

    assert cfg.LEG_ANGLE_NAMES == jo.NAMES and len(cfg.LEG_ANGLE_NAMES) == 8
    assert len(cfg.LEG_NAMES) == 6 == len(set(cfg.LEG_NAMES))
    joints = [j for leg in range(6) for j in cfg.leg_joints(leg)]
    leg_kinds = (cfg.BODY_COXA, cfg.COXA_FEMUR, cfg.FEMUR_TIBIA, cfg.TIBIA_TARSUS, cfg.TARSUS_TIP)
    assert len(joints) == 30 and sorted(joints) == [j for j, kind in enumerate(cfg.TRACKED) if kind in leg_kinds]
    for leg in range(6):
        assert cfg.leg_joints(leg) == jo.leg_joints(leg) and [cfg.TRACKED[j] for j in cfg.leg_joints(leg)] == list(leg_kinds)
    for bad in (-1, 6):
        with pytest.raises(ValueError):
            cfg.leg_joints(bad)


class _Net:
    def __init__(self, calibrated):
        self.calibrated, self.points3d = calibrated, None

    def has_calibration(self):
        return self.calibrated


def test_core_joint_angles_needs_cameras_and_rank_zero(monkeypatch):
    from deepfly3d_amd import distributed as dd
    from deepfly3d_amd.core import Core

    core = Core.__new__(Core)
    core.camNet, core.device, core.is_primary = _Net(False), "cpu", True
    with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
        core.joint_angles()
    core.camNet = None
    with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
        core.joint_angles()
    core.camNet = _Net(True)
    monkeypatch.setattr(dd, "current", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="rank-0"):
        core.joint_angles()
