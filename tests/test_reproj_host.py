"""CPU tests of the suspect-detection search: the float64 oracle's own rules, the argument validation of
df3d_reproj_errors (no device is touched), config.REPROJ_THR, the CLI flag, and Core's error navigation on a fake flag table."""
import ctypes
import math

import numpy as np
import pytest

import reproj_oracle as ro


def _golden(golden_dir, T=4):
    from oracle import geometry as og

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    P = og.projection_matrices(g3["R"], g3["tvec"], g3["intr"])
    X = g3["points3d_wo_procrustes"][:T]
    see = g3["points2d"][:, :T] != 0   # the golden recording's views
    px = np.zeros((7, T, 38, 2))
    for c in range(7):
        for t in range(T):
            for j in range(38):
                u, v, w = ro.project(P[c], X[t, j])
                px[c, t, j] = (v / w, u / w)
    px[~see.all(-1)] = 0.0
    return P, px, X


# ------------------------------------------------------------------------------------------------------------------ oracle
def test_oracle_clean_projections_are_not_flagged(golden_dir):
    P, px, X = _golden(golden_dir)
    err, jmax, mask = ro.reproj_errors(P, px, X, np.full(38, 40.0))
    assert err.max() < 1e-9 and np.all(mask == 0)
    assert np.array_equal(jmax, err.max(axis=0))


def test_oracle_planted_shift_is_flagged(golden_dir):
    P, px, X = _golden(golden_dir)
    c = int(np.flatnonzero(px[:, 2, 5, 0])[1])
    px[c, 2, 5, 1] += 100.0   # 100 px along the columns in one view; X is taken as given
    err, jmax, mask = ro.reproj_errors(P, px, X, np.full(38, 40.0))
    assert abs(err[c, 2, 5] - 100.0) < 1e-6 and abs(jmax[2, 5] - 100.0) < 1e-6
    assert list(mask) == [0, 0, 1 << 5, 0]
    assert np.array_equal(ro.flags(mask, 38)[2], np.arange(38) == 5)


def test_oracle_fewer_than_two_views_give_zero(golden_dir):
    P, px, X = _golden(golden_dir)
    X = X + 5.0   # far from every detection
    for keep in (0, 1):
        q = px.copy()
        views = np.flatnonzero(q[:, 1, 3, 0])
        q[views[keep:], 1, 3] = 0.0
        err, jmax, mask = ro.reproj_errors(P, q, X, np.full(38, 40.0))
        assert np.all(err[:, 1, 3] == 0.0) and jmax[1, 3] == 0.0 and not ro.flags(mask, 38)[1, 3]
    # a camera with one zero coordinate is not a view either
    q = px.copy()
    views = np.flatnonzero(q[:, 0, 0, 0])
    q[views[0], 0, 0, 0] = 0.0
    err, _, _ = ro.reproj_errors(P, q, X, np.full(38, 40.0))
    assert err[views[0], 0, 0] == 0.0 and err[views[1], 0, 0] > 0.0


def test_oracle_point_behind_a_camera_is_inf(golden_dir):
    P, px, X = _golden(golden_dir, T=1)
    j = 0
    c = int(np.flatnonzero(px[:, 0, j, 0])[0])
    # mirror X[0, j] through camera c's centre: w changes sign
    centre = -np.linalg.solve(P[c][:, :3], P[c][:, 3])
    Xb = X.copy()
    Xb[0, j] = centre - (X[0, j] - centre)
    assert ro.project(P[c], Xb[0, j])[2] < 0
    err, jmax, mask = ro.reproj_errors(P, px, Xb, np.full(38, 1e300))
    assert err[c, 0, j] == math.inf and jmax[0, j] == math.inf and ro.flags(mask, 38)[0, j]
    thr = np.full(38, 40.0)
    thr[j] = math.inf   # +inf disables the joint, even for an infinite error
    _, _, mask = ro.reproj_errors(P, px, Xb, thr)
    assert not ro.flags(mask, 38)[0, j]
    # a non-finite point is degenerate: +inf too
    Xn = X.copy()
    Xn[0, j, 1] = np.nan
    err, _, _ = ro.reproj_errors(P, px, Xn, thr)
    assert err[c, 0, j] == math.inf


def test_oracle_threshold_is_strict(golden_dir):
    P, px, X = _golden(golden_dir, T=1)
    px[np.flatnonzero(px[:, 0, 7, 0])[0], 0, 7, 0] += 37.5
    _, jmax, _ = ro.reproj_errors(P, px, X, np.full(38, 40.0))
    thr = np.full(38, math.inf)
    thr[7] = jmax[0, 7]
    assert ro.reproj_errors(P, px, X, thr)[2][0] == 0           # equal: not flagged
    thr[7] = np.nextafter(jmax[0, 7], -math.inf)
    assert ro.reproj_errors(P, px, X, thr)[2][0] == 1 << 7      # one ulp below: flagged
    thr = np.zeros(38)                                          # 0: every joint with a non-zero error
    _, jmax, mask = ro.reproj_errors(P, px, X, thr)
    assert np.array_equal(ro.flags(mask, 38)[0], jmax[0] > 0)


def test_oracle_bit_63_is_the_sign_bit():
    P = np.zeros((2, 3, 4))
    P[:, 2, 3] = 1.0   # w = 1, u = v = 0
    px = np.ones((2, 1, 64, 2))
    _, _, mask = ro.reproj_errors(P, px, np.zeros((1, 64, 3)), np.zeros(64))
    assert mask[0] == -1 and ro.flags(mask, 64).all()


# ------------------------------------------------------------------------------------------------------------------ C entry
def test_reproj_entry_validates_arguments_without_gpu(native_lib):
    lib = native_lib
    p16 = ctypes.c_void_p(4096)
    P = (ctypes.c_double * 96)()
    thr = (ctypes.c_double * 64)(*([40.0] * 64))
    assert lib.df3d_reproj_errors(P, p16, p16, 0, 4, 38, thr, p16, p16, p16, None) == -1 and b"ncam" in lib.df3d_last_error()
    assert lib.df3d_reproj_errors(P, p16, p16, 9, 4, 38, thr, p16, p16, p16, None) == -1 and b"ncam" in lib.df3d_last_error()
    assert lib.df3d_reproj_errors(P, p16, p16, 7, 4, 0, thr, p16, p16, p16, None) == -1 and b"64" in lib.df3d_last_error()
    assert lib.df3d_reproj_errors(P, p16, p16, 7, 4, 65, thr, p16, p16, p16, None) == -1 and b"64" in lib.df3d_last_error()
    assert lib.df3d_reproj_errors(P, p16, p16, 7, -1, 38, thr, p16, p16, p16, None) == -1
    assert lib.df3d_reproj_errors(None, None, None, 7, 0, 38, None, None, None, None, None) == 0   # no frames: nothing to do
    for i in range(6):   # P, points, X, thresholds, err, mask; jmax may be NULL
        args = [P, p16, p16, thr, p16, p16]
        args[i] = None
        rc = lib.df3d_reproj_errors(args[0], args[1], args[2], 7, 4, 38, args[3], args[4], p16, args[5], None)
        assert rc == -1 and b"null" in lib.df3d_last_error(), i
    for bad in (float("nan"), -1.0, -0.5e-300):
        t = (ctypes.c_double * 64)(*([40.0] * 64))
        t[37] = bad
        assert lib.df3d_reproj_errors(P, p16, p16, 7, 4, 38, t, p16, p16, p16, None) == -1 and b"thresholds" in lib.df3d_last_error()


def test_reproj_thresholds_config():
    from deepfly3d_amd.config import REPROJ_THR

    assert REPROJ_THR.dtype == np.float64 and REPROJ_THR.shape == (38,) and np.all(REPROJ_THR == 40.0)


def test_cli_correct_only_flagged_needs_auto_correct():
    from deepfly3d_amd.cli import parse_cli_args

    args = parse_cli_args(["/tmp/x", "--auto-correct", "--correct-only-flagged"])
    assert args.auto_correct and args.correct_only_flagged
    assert parse_cli_args(["/tmp/x", "--auto-correct"]).correct_only_flagged is False
    with pytest.raises(SystemExit) as e:
        parse_cli_args(["/tmp/x", "--correct-only-flagged"])
    assert e.value.code == 2


def test_flagged_only_is_not_a_pictorial_parameter():
    import inspect

    from deepfly3d_amd.config import PICTORIAL_DEFAULTS
    from deepfly3d_amd.core import Core

    assert "flagged_only" not in PICTORIAL_DEFAULTS
    assert inspect.signature(Core.auto_correct).parameters["flagged_only"].default is False


# ------------------------------------------------------------------------------------------------------------------ Core search
class _Cam:
    def __init__(self, cam_id):
        self.cam_id, self.P = cam_id, np.eye(3, 4)


class _Net:
    """A calibrated camera network of `ncam` cameras and one joint whose detections encode the frame id (row = t + 1)."""

    def __init__(self, T, ncam=2, calibrated=True):
        self.points2d = np.zeros((ncam, T, 1, 2))
        self.points2d[:, :, 0, 0] = np.arange(1, T + 1)
        self.cam_list = [_Cam(c) for c in range(ncam)]
        self.calibrated = calibrated

    def has_calibration(self):
        return self.calibrated


@pytest.fixture
def fake_core(monkeypatch):
    """(make(T, flagged), calls): a Core on a fake camera network whose ops.reprojection_errors answers from a flag table
    {frame: mask}, with err[c, t, 0] = 10 c + 1 on flagged frames; calls records the frame ids of every evaluation."""
    import torch

    from deepfly3d_amd import _native, ops
    from deepfly3d_amd.core import Core

    calls = []
    table = {}

    def fake(P, px, X=None, thresholds=None, frames=None):
        ids = (px[0, :, 0, 0] - 1).long()
        calls.append(ids.tolist())
        mask = torch.tensor([table.get(int(t), 0) for t in ids], dtype=torch.int64)
        err = torch.zeros((px.shape[0], len(ids), 1), dtype=torch.float64)
        err[:, mask != 0, 0] = (10.0 * torch.arange(px.shape[0], dtype=torch.float64) + 1.0)[:, None]
        return err, err.max(dim=0).values, mask

    monkeypatch.setattr(ops, "reprojection_errors", fake)
    monkeypatch.setattr(_native, "require_gpu", lambda: 1)

    def make(T, flagged, ncam=2):
        table.clear()
        table.update({t: 1 for t in flagged})
        core = Core.__new__(Core)
        core.camNet, core.device, core.is_primary, core.max_img_id = _Net(T, ncam), "cpu", True, T - 1
        return core

    return make, calls


def test_core_next_and_prev_error_order(fake_core):
    make, calls = fake_core
    core = make(50, [5, 17, 30])
    assert core.next_error(0) == 5 and core.next_error(5) == 17 and core.next_error(17) == 30 and core.next_error(30) is None
    assert core.prev_error(49) == 30 and core.prev_error(30) == 17 and core.prev_error(17) == 5 and core.prev_error(5) is None
    assert core.next_error(-1) == 5 and core.prev_error(0) is None   # an empty range evaluates nothing
    assert calls[-1] == list(range(0, 50))
    assert core.next_error_in_range([]) is None
    assert make(50, []).next_error(0) is None


def test_core_next_error_chunks_grow_and_stop_early(fake_core):
    make, calls = fake_core
    T = 300_000
    for flag, sizes in ((1023, [1024]), (1024, [1024, 2048]), (3071, [1024, 2048]), (3072, [1024, 2048, 4096])):
        calls.clear()
        assert make(T, [flag, T - 1]).next_error_in_range(range(T)) == flag
        assert [len(c) for c in calls] == sizes, flag
    calls.clear()
    assert make(T, [T - 1]).next_error_in_range(range(T - 1)) is None
    sizes = [len(c) for c in calls]
    assert sizes[:7] == [1024 << k for k in range(7)] and all(s == 65536 for s in sizes[7:-1]) and sum(sizes) == T - 1
    assert [i for c in calls for i in c] == list(range(T - 1))
    # backwards over the boundaries of chunks counted from the end
    calls.clear()
    assert make(T, [T - 1 - 1024 - 5]).prev_error(T - 1) == T - 1 - 1024 - 5
    assert [len(c) for c in calls] == [1024, 2048] and calls[0][0] == T - 2


def test_core_non_contiguous_range(fake_core):
    make, calls = fake_core
    core = make(200, [3, 2, 150])
    assert core.next_error_in_range([7, 3, 100, 2]) == 3
    assert core.next_error_in_range(iter([150, 2])) == 150
    assert core.next_error_in_range(x for x in (9, 8, 199)) is None
    assert calls[0] == [7, 3, 100, 2]
    with pytest.raises(IndexError):
        core.next_error_in_range([1, 200])
    with pytest.raises(IndexError):
        core.next_error_in_range([-1])


def test_core_joint_queries(fake_core):
    from deepfly3d_amd.camera_network import Camera

    make, _ = fake_core
    core = make(20, [4], ncam=3)
    assert core.joint_has_error(4, 0) and not core.joint_has_error(5, 0)
    assert core.get_joint_reprojection_error(4, 0) == 21.0 and core.get_joint_reprojection_error(5, 0) == 0.0
    assert core.get_joint_reprojection_error(4, 0, camNet=[0, 1]) == 11.0
    assert core.get_joint_reprojection_error(4, 0, camNet=[Camera(0, None)]) == 1.0
    assert core.get_joint_reprojection_error(4, 0, camNet=core.camNet) == 21.0
    assert core.reprojection_errors().shape == (3, 20, 1) and core.reprojection_errors([4, 2])[:, :, 0].tolist() == [[1, 0], [11, 0], [21, 0]]


def test_core_queries_need_cameras_and_rank_zero(fake_core, monkeypatch):
    from deepfly3d_amd import distributed as dd

    make, _ = fake_core
    core = make(10, [])
    core.camNet.calibrated = False
    with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
        core.next_error(0)
    core.camNet = None
    with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
        core.joint_has_error(0, 0)
    core = make(10, [])
    core.is_primary = False
    monkeypatch.setattr(dd, "current", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="rank-0"):
        core.prev_error(5)
