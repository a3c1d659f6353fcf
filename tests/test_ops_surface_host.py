"""Host tests of deepfly3d_amd/ops.py as a module: no top-level name is bound twice, the public surface is the one recorded in
tests/golden/ops_api.json, and the argument checks that the families share refuse and accept what they say."""
import ast
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_no_module_level_name_is_bound_twice():
    with open(os.path.join(ROOT, "deepfly3d_amd", "ops.py")) as f:
        tree = ast.parse(f.read())
    bound = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            bound.append(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign)):
            targets = node.targets if isinstance(node, ast.Assign) else [node.target]
            bound += [n.id for t in targets for n in ast.walk(t) if isinstance(n, ast.Name)]
    twice = sorted({n for n in bound if bound.count(n) > 1})
    assert not twice, f"bound more than once at module level (the last one wins for every caller): {twice}"


def test_public_surface_is_the_recorded_one():
    from deepfly3d_amd import ops

    with open(os.path.join(ROOT, "tests", "golden", "ops_api.json")) as f:
        want = json.load(f)
    got = {n: (str(inspect.signature(o)) if callable(o) else type(o).__name__) for n, o in vars(ops).items()
           if not n.startswith("_") and not isinstance(o, types.ModuleType)}
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    for private in ("_gait_fps", "_need_grid", "_coxa_medians", "_distributions", "_stream", "_need", "_call"):   # used from outside the module
        assert callable(getattr(ops, private)), private


def test_integer_and_number():
    from deepfly3d_amd import ops

    lo, hi = 2, 8
    for bad in (True, 1.0, lo - 1, hi + 1, "3", None, np.float64(3.0)):
        with pytest.raises(ValueError, match=r"n must be an integer in \[2, 8\] \(it is "):
            ops._integer(bad, lo, hi, "n")
    for good in (lo, hi, np.int64(lo), np.int32(hi)):
        got = ops._integer(good, lo, hi, "n")
        assert type(got) is int and got == int(good)
    for bad in (True, "1", None, [1.0], 1j):
        with pytest.raises(ValueError, match=r"x must be a number \(it is "):
            ops._number(bad, "x")
    for good in (1, 2.5, np.float32(0.5), np.int64(-3), NAN, float("inf")):
        got = ops._number(good, "x")
        assert type(got) is float and (got == float(good) or np.isnan(got))
    for bad in (True, "1", 0, -1.0, NAN, float("inf")):
        with pytest.raises(ValueError, match=r"fps must be a finite number > 0 \(it is "):
            ops._number(bad, "fps", positive=True)
    assert ops._number(np.float32(100.0), "fps", positive=True) == 100.0 and ops._gait_fps(25) == 25.0


def test_per_joint_values():
    from deepfly3d_amd import ops

    J = 5
    default = np.full(38, 20.0)
    for bad in ("x", True, np.array([object()] * J), [None], object()):
        with pytest.raises(ValueError, match="tau must be a number or one number per joint"):
            ops._per_joint(bad, default, "tau")
    for bad in ([], -1.0, [1.0, -2.0], NAN, [1.0, NAN]):
        with pytest.raises(ValueError, match="tau must be >= 0 and not NaN"):
            ops._per_joint(bad, default, "tau")
    with pytest.raises(ValueError, match="lam must be >= 0 and finite"):
        ops._per_joint(float("inf"), default, "lam", finite=True)
    assert ops._per_joint(float("inf"), default, "tau").tolist() == [float("inf")]
    one, each, own = ops._per_joint(3, default, "tau"), ops._per_joint(list(range(J)), default, "tau"), ops._per_joint(None, default, "tau")
    assert one.dtype == each.dtype == own.dtype == np.float64
    assert one.tolist() == [3.0] and each.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and np.array_equal(own, default) and own is not default

    assert ops._broadcast_per_joint(one, J, "tau").tolist() == [3.0] * J
    wide = ops._broadcast_per_joint(each, J, "tau")
    assert wide.tolist() == each.tolist() and wide.flags["C_CONTIGUOUS"] and wide.shape == (J,)
    with pytest.raises(ValueError, match=r"tau must hold one value, or one per joint \(5\)$"):
        ops._broadcast_per_joint(np.zeros(4), J, "tau")
    with pytest.raises(ValueError, match=r"tau must hold one value, or one per joint \(5\) \(config.ROBUST_TAU is for 38\)$"):
        ops._broadcast_per_joint(own, J, "tau", "ROBUST_TAU")
    assert ops._broadcast_per_joint(own, 38, "tau", "ROBUST_TAU").shape == (38,)


def test_camera_matrices():
    from deepfly3d_amd import ops

    ncam = 3
    P = np.arange(ncam * 12, dtype=np.float32).reshape(ncam, 3, 4)
    for given in (P, torch.from_numpy(P), torch.from_numpy(P).double(), P.tolist()):
        got = ops._camera_matrices(given, ncam)
        assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, P)
    for bad in (np.zeros((ncam + 1, 3, 4)), np.zeros((ncam, 4, 3)), np.zeros((3, 4)), torch.zeros((ncam - 1, 3, 4))):
        with pytest.raises(ValueError, match=r"P must be \[ncam, 3, 4\]"):
            ops._camera_matrices(bad, ncam)


def test_body_frame_argument():
    from deepfly3d_amd import ops

    T, cpu = 5, torch.device("cpu")
    assert ops._body_frames("recording", T, cpu) is None and ops._body_frames("per_frame", T, cpu) is None
    assert ops._body_frames("recording", T, cpu, per_frame_allowed=False) is None
    with pytest.raises(ValueError, match='body_frame must be "recording", "per_frame" or a'):
        ops._body_frames("per_frame", T, cpu, per_frame_allowed=False)
    with pytest.raises(ValueError, match='body_frame must be "recording", "per_frame" or a'):
        ops._body_frames("thorax", T, cpu)
    for bad in (np.zeros((2, 3, 3)), np.eye(4), np.zeros(3)):
        with pytest.raises(ValueError, match=r"an explicit body_frame must be \[3, 3\] or \[T, 3, 3\] with T = 5"):
            ops._body_frames(bad, T, cpu)
    with pytest.raises(ValueError, match="one frame"):
        ops._body_frames(np.zeros((T, 3, 3)), T, cpu, per_frame_allowed=False, text=("no string", "one frame"))
    for given, n in ((np.eye(3), 1), (np.eye(3)[None], 1), (torch.eye(3, dtype=torch.float32), 1), (np.zeros((T, 3, 3)), T)):
        frames = ops._body_frames(given, T, cpu)
        assert tuple(frames.shape) == (n, 3, 3) and frames.dtype == torch.float64 and frames.is_contiguous()
    given = torch.eye(3, dtype=torch.float64)[None]
    assert ops._fill_body_frames(given, "recording", None) is given   # an explicit frame is used as given: nothing is computed


def test_tensor_checks_refuse_before_any_device_work(native_lib):
    from deepfly3d_amd import ops

    pose = torch.zeros((4, 38, 3), dtype=torch.float64)   # a CPU tensor
    with pytest.raises(ValueError, match=r"points3d must be a torch.float64 CUDA tensor of shape \[T, 38, 3\]"):
        ops._need_tensor(pose, torch.float64, (38, 3), "points3d")
    with pytest.raises(ValueError, match=r"labels must be a torch.int32 CUDA tensor of shape \[T\]$"):
        ops._need_tensor(pose, torch.int32, (), "labels")
    for call in (ops.body_frame, ops.joint_angles, ops.segment_length_medians, ops.fit_legs, ops.recording_frame, ops.pose_outliers):
        with pytest.raises(ValueError, match=r"points3d must be a torch.float64 CUDA tensor of shape \[T, 38, 3\]"):
            call(pose)
    with pytest.raises(ValueError, match="points2d_px must be a contiguous torch.float64 CUDA tensor"):
        ops._need_points2d_px(torch.zeros((3, 4, 5, 2), dtype=torch.float64))
