"""CPU tests of the treadmill model: the oracle on the planted ball -- centre, radius, rotation under the
chord-versus-tangent bound, the straight path of a forward walk and the turn of a pure yaw --, its refusals and its kernel-form sums
inside their bound, and every refusal of ops, Core and the command line that comes before the device."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gait_oracle as go  # noqa: E402
import treadmill_oracle as to  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
TREADMILL_KEYS = ["treadmill_ball_center", "treadmill_ball_radius", "treadmill_ball_rms", "treadmill_ball_count", "treadmill_ball_status",
                  "treadmill_rotation", "treadmill_legs", "treadmill_residual", "treadmill_fictive", "treadmill_path", "treadmill_skipped",
                  "treadmill_params", "treadmill_fps"]


# ------------------------------------------------------------------------------------------------------------------ the planted ball
@pytest.mark.parametrize("kind", ["walk", "yaw"])
def test_oracle_recovers_the_planted_ball(golden_dir, kind):
    planted = to.planted_ball(go.planted_pose(golden_dir), kind)
    r = to.treadmill(planted["X"], to.PLANTED["fps"], planted["F"], planted["medians"], states=planted["states"])
    worst, bound = to.check_planted(r, planted, kind)
    print(f"{kind}: rotation off by {worst:.3e} relative, chord bound {bound:.3e}")
    if kind == "walk":   # the figures of the issue: |omega| = 4.09 rad/s, w = 2, fps = 100
        assert abs(to.chord_bound(4.09, 100.0, 2) - 1.115e-3) < 1e-6 and 0.5 * bound < worst <= bound
        # gait's own states, from the anterior velocity: stance wherever the planted states say so, and every tip is on the sphere
        own = to.treadmill(planted["X"], to.PLANTED["fps"], planted["F"], planted["medians"])
        assert np.all(own["states"][planted["states"] == 0] == 0) and own["fit"]["status"] == 0
        assert np.linalg.norm(own["fit"]["center"] - planted["center"]) <= 1e-9 and abs(own["fit"]["radius"] - planted["radius"]) <= 1e-9


def test_known_radius_and_noise(golden_dir):
    """The algebraic radius is biased low by noise; the known-radius centre is nearer, and its steps contract."""
    planted = to.planted_ball(go.planted_pose(golden_dir))
    b, _ = to.body_tips(planted["X"], 100.0, planted["F"], planted["medians"])
    clean = to.fit_ball(b, planted["states"], radius=planted["radius"])
    assert clean["status"] == 0 and len(clean["steps"]) == to.ITERATIONS and clean["steps"][-1] <= 1e-12
    assert np.linalg.norm(clean["center"] - planted["center"]) <= to.known_radius_bar(b, planted["states"], clean) + 1e-12
    noisy = b + np.random.default_rng(0).normal(0.0, 0.05, b.shape)
    free, known = to.fit_ball(noisy, planted["states"]), to.fit_ball(noisy, planted["states"], radius=planted["radius"])
    assert free["status"] == known["status"] == 0 and free["radius"] < planted["radius"] and known["radius"] == planted["radius"]
    assert np.linalg.norm(known["center"] - planted["center"]) < np.linalg.norm(free["center"] - planted["center"])
    assert known["steps"][-1] <= 1e-12 and to.known_radius_bar(noisy, planted["states"], known) < 1e-9
    assert 0.04 < known["rms"] < 0.06   # the planted noise


def test_refusals_of_the_fit():
    rng = np.random.default_rng(1)
    c, R = np.array([0.3, -0.2, -6.0]), 5.0
    d = rng.normal(size=(40, 6, 3))
    d[..., 2] = np.abs(d[..., 2]) + 0.5   # a cap of the sphere, towards the origin
    b = c + R * d / np.linalg.norm(d, axis=-1, keepdims=True)
    states = np.zeros((40, 6), dtype=np.int32)
    fit = to.fit_ball(b, states)
    assert fit["status"] == 0 and fit["count"] == 240 and np.linalg.norm(fit["center"] - c) < 1e-12 and abs(fit["radius"] - R) < 1e-12
    for count, radius, status in ((3, None, to.REFUSED), (3, R, to.START_BELOW), (2, R, to.REFUSED), (0, None, to.REFUSED)):
        few = np.ones((40, 6), dtype=np.int32)
        few.reshape(-1)[:count] = 0
        fit = to.fit_ball(b, few, radius)
        assert fit["status"] == status and fit["count"] == count and np.isnan(fit["center"]).all() == bool(status & to.REFUSED)
    # a flat stance set: no algebraic centre; with a known radius the fit starts beyond the tips and lands on the sphere
    flat = b.copy()
    flat[..., 2] = -2.0
    rho = R * R - (c[2] + 2.0) ** 2   # the circle where the sphere cuts the plane z = -2
    flat[..., :2] = c[:2] + np.sqrt(rho) * d[..., :2] / np.linalg.norm(d[..., :2], axis=-1, keepdims=True)
    assert to.fit_ball(flat, states)["status"] == to.REFUSED
    fit = to.fit_ball(flat, states, radius=R)
    assert fit["status"] == to.START_BELOW and np.linalg.norm(fit["center"] - c) < 1e-9 and fit["rms"] < 1e-9
    # all unknown, or every tip missing: no samples
    assert to.fit_ball(b, np.full((40, 6), -1, dtype=np.int32))["status"] == to.REFUSED
    assert to.fit_ball(np.full_like(b, NAN), states)["count"] == 0


def test_kernel_form_sums_lie_within_the_summation_bound():
    T = 2 * to.S // 6 + 50   # three slices, the last one partial
    rng = np.random.default_rng(2)
    b = rng.normal(size=(T, 6, 3)) + np.array([0.0, 0.0, -3.0])
    b[rng.random((T, 6)) < 0.05] = NAN
    states = to.random_states(T, seed=3)
    exact, form = to.ball_sums(b, states), to.sums_kernel_form(b, states)
    assert exact[0] == form[0] == to.samples(b, states).sum()
    keep = to.samples(b, states).reshape(-1)
    q = np.abs(b.reshape(-1, 3)[keep] - exact[1:4] / exact[0])
    w = (q * q).sum(axis=1)
    big = np.concatenate([np.abs(b.reshape(-1, 3)[keep]).sum(axis=0), (q[:, :1] * np.c_[q, np.ones(len(q))]).sum(axis=0),
                          (q[:, 1:2] * np.c_[q[:, 1:], np.ones(len(q))]).sum(axis=0), (q[:, 2:] * np.c_[q[:, 2:], np.ones(len(q))]).sum(axis=0),
                          (q * w[:, None]).sum(axis=0), [w.sum()]])
    # n terms in any order: (n - 1) u times the sum of their magnitudes; the centred terms also see the two means differ by that much
    assert np.all(np.abs(form[1:] - exact[1:]) <= 4.0 * (exact[0] + 8.0) * to.U * big)


def test_rotation_by_hand():
    c, R = np.array([0.0, 0.0, -5.0]), 5.0
    omega = np.array([0.3, -4.0, 0.7])
    rng = np.random.default_rng(4)
    d = rng.normal(size=(8, 6, 3))
    b = c + R * d / np.linalg.norm(d, axis=-1, keepdims=True)
    v = np.cross(omega, b - c)
    states = np.zeros((8, 6), dtype=np.int32)
    states[1, 1:] = 1                   # one stance leg: the spin about its radius is free
    states[2, 2:] = 1                   # two legs
    states[3, 2:] = 1
    b[3, 1] = c + 0.5 * (b[3, 0] - c)   # two legs with parallel radii
    v[3, 1] = np.cross(omega, b[3, 1] - c)
    states[4] = -1                      # nobody in stance
    v[5, 2] = NAN                       # a leg without a velocity is left out
    r = to.ball_rotation(b, v, states, c, R)
    assert r["legs"].tolist() == [6, 1, 2, 2, 0, 5, 6, 6]
    assert np.isnan(r["rotation"][[1, 3, 4]]).all() and np.isnan(r["fictive"][[1, 3, 4]]).all() and np.isnan(r["residual"][[1, 3, 4]]).all()
    ok = [0, 2, 5, 6, 7]
    assert np.all(np.linalg.norm(r["rotation"][ok] - omega, axis=1) <= r["bar"][ok] + 1e-13) and np.all(r["residual"][ok] <= 1e-12)
    # the fly stands on top of the ball: u = (0, 0, 1), s = -(omega x R u)
    assert np.allclose(r["fictive"][ok], [-omega[1] * R, omega[0] * R, -omega[2]], rtol=0, atol=1e-12)
    assert np.isnan(to.ball_rotation(b, v, states, np.full(3, NAN), NAN)["rotation"]).all()   # a refused ball
    assert to.ball_rotation(b, v, states, c, R, min_legs=3)["legs"].tolist() == r["legs"].tolist()
    assert np.isnan(to.ball_rotation(b, v, states, c, R, min_legs=3)["rotation"][2]).all()


def test_path_by_hand():
    fps = 10.0
    quarter = np.pi / 2 * fps
    f = np.array([[10.0, 0.0, 0.0], [10.0, 0.0, quarter], [NAN, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, -quarter], [10.0, 0.0, 0.0]])
    r = to.fictive_path(f, fps)
    want = [[0, 0, 0], [1, 0, 0], [2, 0, np.pi / 2], [2, 0, np.pi / 2], [2, 1, np.pi / 2], [1, 1, 0]]
    assert r["skipped"] == 1 and np.allclose(r["path"], want, rtol=0, atol=1e-15)
    assert to.fictive_path(np.zeros((0, 3)), fps)["path"].shape == (0, 3)


def test_tips_windows_and_missing():
    T, fps = 7, 50.0
    X = np.random.default_rng(1).normal(size=(T, 38, 3))
    X[3, go.TIPS[2]] = 0.0
    F, medians = np.eye(3), to.coxa_medians(X)
    b, v = to.body_tips(X, fps, F, medians, 2)
    o = to.origin(medians)
    assert np.isnan(b[3, 2]).all() and np.isnan(v[[1, 5], 2]).all() and np.isfinite(np.delete(b, 2, axis=1)).all()
    assert np.array_equal(b[0, 0], X[0, go.TIPS[0]] - o)            # neither mirrored nor relative to the coxa
    assert np.allclose(v[0, 0], (X[2, go.TIPS[0]] - X[0, go.TIPS[0]]) * (fps / 2), rtol=1e-15, atol=0)   # the clipped window
    assert np.isnan(to.body_tips(X[:1], fps, F, medians)[1]).all()   # one frame: an empty window
    assert np.array_equal(v[..., 0], go.tip_kinematics(X, fps, F, 2)[1][..., 0], equal_nan=True)   # the anterior velocity is gait's own
    bad = F.copy()
    bad[1, 1] = INF
    assert np.isnan(to.body_tips(X, fps, bad, medians)[0]).all()


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_constants_agree():
    from deepfly3d_amd import config

    ours = (config.BALL_FIT_ITERATIONS, config.BALL_PIVOT_MIN, config.BALL_MIN_LEGS, config.BALL_FRAME_PIVOT_MIN)
    assert ours == (to.ITERATIONS, to.PIVOT_MIN, to.MIN_LEGS, to.FRAME_PIVOT_MIN)
    assert config.BALL_MIN_LEGS_RANGE == (2, 6) and config.BALL_FIT_ITERATIONS_RANGE == (1, 64)
    source = open(os.path.join(ROOT, "deepfly3d_amd", "csrc", "treadmill.hip")).read()
    assert re.search(rf"constexpr int SLICE = {to.S};", source) and to.B == to.SCAN_BLOCK ** 2 == 65536
    shared = open(os.path.join(ROOT, "deepfly3d_amd", "csrc", "gait_dev.h")).read()
    assert f"constexpr int THREADS = {to.THREADS};" in shared
    # the window, the missing rule and the scan scaffold are shared through the header, not copied
    gait = open(os.path.join(ROOT, "deepfly3d_amd", "csrc", "gait.hip")).read()
    for text in (source, gait):
        assert '#include "gait_dev.h"' in text and "bool missing(" not in text and "lds[t - o]" not in text
    assert "bool missing(" in shared and "lds[t - o]" in shared and "void window(" in shared


def test_built_without_contraction():
    from deepfly3d_amd import build

    assert build.FILE_FLAGS["treadmill.hip"] == ["-ffp-contract=off"] and build.FILE_FLAGS["gait.hip"] == ["-ffp-contract=off"]


def test_ops_refusals_come_before_any_work():
    from deepfly3d_amd import ops

    assert ops.treadmill_params() == (None, to.MIN_LEGS, to.ITERATIONS) and ops.treadmill_params(5, 3, 2) == (5.0, 3, 2)
    for radius in (0.0, -1.0, NAN, INF, "5", True):
        with pytest.raises(ValueError, match="radius must be a finite number > 0"):
            ops.treadmill_params(radius)
        with pytest.raises(ValueError, match="radius must be a finite number > 0"):
            ops.treadmill(None, 100.0, radius=radius)   # before the pose is looked at
    for min_legs in (1, 7, 2.0, True):
        with pytest.raises(ValueError, match=r"min_legs must be an integer in \[2, 6\]"):
            ops.treadmill(None, 100.0, min_legs=min_legs)
    for iterations in (0, 65, 1.5):
        with pytest.raises(ValueError, match=r"iterations must be an integer in \[1, 64\]"):
            ops.treadmill(None, 100.0, radius=5.0, iterations=iterations)
    with pytest.raises(ValueError, match=r"half_window must be an integer in \[1, 64\]"):
        ops.treadmill(None, 100.0, half_window=0)
    with pytest.raises(ValueError, match="on must be above off"):
        ops.treadmill(None, 100.0, on=0.0, off=1.0)
    with pytest.raises(ValueError, match="with states handed in they have nothing to decide"):
        ops.treadmill(None, 100.0, states=np.zeros((3, 6)), on=1.0)
    with pytest.raises(ValueError, match="fps must be a finite number > 0"):
        ops.treadmill(None, 0.0)
    with pytest.raises(ValueError, match="points3d must be a torch.float64 CUDA tensor"):
        ops.treadmill(np.zeros((3, 38, 3)), 100.0)
    for fn, args in ((ops.fit_ball, (None, None)), (ops.ball_rotation, (None, None, None, None))):
        with pytest.raises(ValueError, match="tips must be a torch.float64 CUDA tensor"):
            fn(*args)
    with pytest.raises(ValueError, match="fictive must be a torch.float64 CUDA tensor"):
        ops.fictive_path(None, 100.0)
    assert list(inspect.signature(ops.fit_ball).parameters)[:3] == ["tips", "states", "radius"]
    assert list(inspect.signature(ops.ball_rotation).parameters) == ["tips", "vel", "states", "ball", "min_legs"]
    assert list(inspect.signature(ops.fictive_path).parameters) == ["fictive", "fps"]
    assert list(inspect.signature(ops.treadmill).parameters)[:5] == ["points3d", "fps", "body_frame", "states", "radius"]
    assert [f.name for f in ops.TreadmillResult.__dataclass_fields__.values()][:4] == ["tip", "vel", "states", "ball"]


def test_cli_flags(capsys):
    from deepfly3d_amd import cli

    args = cli.parse_cli_args(["x"])
    assert args.treadmill is False and args.ball_radius is None
    args = cli.parse_cli_args(["x", "--treadmill", "--ball-radius", "4.5", "--gait", "--repair-pose", "--skip-pose-estimation"])
    assert args.treadmill and args.ball_radius == 4.5 and args.gait and args.repair_pose
    assert cli.parse_cli_args(["x", "--treadmill"]).ball_radius is None
    for argv, message in ((["x", "--ball-radius", "5"], "--ball-radius sets the radius of --treadmill: it needs --treadmill"),
                          (["x", "--treadmill", "--ball-radius", "0"], "radius must be a finite number > 0"),
                          (["x", "--treadmill", "--ball-radius=-2"], "radius must be a finite number > 0"),
                          (["x", "--treadmill", "--ball-radius", "nan"], "radius must be a finite number > 0"),
                          (["x", "--treadmill", "--ball-radius", "big"], "invalid float value")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err), argv
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--treadmill" in text and "--ball-radius MM" in text and "nobody has measured on a recording" in text


def test_core_refusals(tmp_path, golden_dir):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    folder = str(folder)
    config.pop("image_shape", None)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    with pytest.raises(RuntimeError, match="treadmill needs calibrated cameras"):
        core.treadmill()
    with pytest.raises(RuntimeError, match="treadmill needs calibrated cameras"):
        core.treadmill(repair=True)
    for kw, message in ((dict(radius=0.0), "radius must be a finite number"), (dict(radius=NAN), "radius must be a finite number"),
                        (dict(min_legs=1), "min_legs must be an integer"), (dict(half_window=65), "half_window must be an integer"),
                        (dict(on=1.0, off=2.0), "on must be above off"), (dict(fps=-1.0), "fps must be a finite number")):
        with pytest.raises(ValueError, match=message):   # before the cameras are asked for
            core.treadmill(**kw)
    named = list(inspect.signature(Core.treadmill).parameters.values())
    assert [p.name for p in named] == ["self", "fps", "radius", "on", "off", "half_window", "min_legs", "repair"]
    assert named[-1].default is False   # the last keyword, as on the six other kinematic methods
    with pytest.raises(ValueError, match="ball_radius belongs to treadmill: it needs treadmill=True"):
        core.save(ball_radius=5.0)
    with pytest.raises(ValueError, match="radius must be a finite number"):
        core.save(treadmill=True, ball_radius=-5.0)
    save = inspect.signature(Core.save).parameters
    assert save["treadmill"].default is False and save["ball_radius"].default is None
    assert list(Core._TREADMILL_KEYS) == TREADMILL_KEYS
    config.pop("image_shape", None)
