"""-m gpu tests of the tracking of the 2-D detections (csrc/track.hip): choice and cost equal the int64 oracle
(tests/track_oracle.py) exactly, at every block size."""
import os
import pickle

import numpy as np
import pytest
import torch

import track_cases as tc
import track_oracle as to
from oracle import geometry as og

pytestmark = pytest.mark.gpu

IMAGE_SHAPE = [960, 480]   # [W, H], as Core carries it
BLOCKS = (1, 2, 5, 16, 64)


def _device(arrays, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _track(ops, peaks, cuda, **params):
    r = ops.track_peaks(*_device(peaks, cuda), IMAGE_SHAPE, **params)
    return r.choice.cpu().numpy(), r.cost.cpu().numpy()


@pytest.mark.parametrize("K", [1, 2, 3, 10, 16])
def test_small_cases_equal_the_oracle(native_lib, cuda, K):
    """C = 2, J = 3, every block size with the recording lengths round it: tie-heavy inputs, counts from 0 to beyond K, NaN and infinities
    in values and coordinates."""
    from deepfly3d_amd import ops

    wanted = {}
    for block in BLOCKS:
        for T in sorted({1, 2, 3, block - 1, block, block + 1, 2 * block + 1, 70}):
            peaks = tc.tie_heavy(1000 * K + T, 2, T, 3, K)
            if T not in wanted:
                wanted[T] = to.solve(*peaks, tc.IMAGE_HW)
            choice, cost = _track(ops, peaks, cuda, block_frames=block)
            assert choice.dtype == np.int32 and cost.dtype == np.int64 and choice.shape == (2, T, 3) and cost.shape == (2, 3)
            assert np.array_equal(cost, wanted[T][1]), (K, block, T)
            assert np.array_equal(choice, wanted[T][0]), (K, block, T)
    assert any(w[0].any() for w in wanted.values()) or K == 1
    # other weights and another truncation, once
    peaks = tc.tie_heavy(77 + K, 2, 37, 3, K)
    choice, cost = _track(ops, peaks, cuda, tau=11.0, w_motion=0.375, w_value=2.5, block_frames=5)
    want = to.solve(*peaks, tc.IMAGE_HW, 11.0, 0.375, 2.5)
    assert np.array_equal(cost, want[1]) and np.array_equal(choice, want[0])


@pytest.fixture(scope="module")
def real_layout():
    peaks = tc.tie_heavy(5, 7, 300, 19, 10)
    return peaks, to.solve(*peaks, tc.IMAGE_HW)


def test_the_real_layout(native_lib, cuda, real_layout):
    from deepfly3d_amd import ops

    peaks, (want_choice, want_cost) = real_layout
    choice, cost = _track(ops, peaks, cuda)
    assert np.array_equal(cost, want_cost) and np.array_equal(choice, want_choice)
    assert 0.2 < (choice != 0).mean() < 0.9   # the case does choose


def test_every_block_size_and_every_run_give_the_same_bits(native_lib, cuda, real_layout):
    from deepfly3d_amd import ops

    peaks, (want_choice, want_cost) = real_layout
    dev = _device(peaks, cuda)
    for block in (1, 2, 5, 16, 64, 256, 299, 300, 301, 4096):
        r = ops.track_peaks(*dev, IMAGE_SHAPE, block_frames=block)
        assert r.params == (30.0, 1.0, 1.0, block)
        assert np.array_equal(r.choice.cpu().numpy(), want_choice) and np.array_equal(r.cost.cpu().numpy(), want_cost), block
    a, b = ops.track_peaks(*dev, IMAGE_SHAPE), ops.track_peaks(*dev, IMAGE_SHAPE)
    assert torch.equal(a.choice, b.choice) and torch.equal(a.cost, b.cost)
    assert torch.equal(a.cost_float, a.cost.double() / 2.0 ** 20)
    empty = ops.track_peaks(*(t[:, :0].contiguous() for t in dev), IMAGE_SHAPE)
    assert tuple(empty.choice.shape) == (7, 0, 19) and not empty.cost.any()


def test_a_long_recording(native_lib, cuda):
    """20 000 frames of 133 chains: 79 blocks of the default size, 5 of the largest."""
    from deepfly3d_amd import ops

    peaks = tc.tie_heavy(9, 7, 20000, 19, 4)
    want_choice, want_cost = to.solve(*peaks, tc.IMAGE_HW)
    dev = _device(peaks, cuda)
    for block in (256, 4096):
        r = ops.track_peaks(*dev, IMAGE_SHAPE, block_frames=block)
        assert np.array_equal(r.cost.cpu().numpy(), want_cost) and np.array_equal(r.choice.cpu().numpy(), want_choice), block


def test_the_planted_distractor(native_lib, cuda):
    from deepfly3d_amd import ops

    count, pts, val, truth = tc.planted()
    assert int((truth != 0).sum()) >= truth.size // 5
    choice, cost = _track(ops, (count, pts, val), cuda)
    assert int((choice != truth).sum()) == 0
    want = to.solve(count, pts, val, tc.IMAGE_HW)
    assert np.array_equal(choice, want[0]) and np.array_equal(cost, want[1])


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0]], ids=["identity", "rev"])
def test_tracked_points2d(native_lib, cuda, order):
    from deepfly3d_amd import ops

    T, K = 9, 5
    count, pts, val = tc.tie_heavy(3, 7, T, 19, K, dirty=False)
    pts[..., 0] += (np.arange(K) / 1024.0).astype(np.float32)
    d_count, d_pts, d_val = _device((count, pts, val), cuda)
    points2d = ops.relayout_19_to_38(d_pts[:, :, :, 0].contiguous(), order)
    r = ops.track_peaks(d_count, d_pts, d_val, IMAGE_SHAPE)
    choice = r.choice.cpu().numpy()
    assert choice.any()
    out = ops.tracked_points2d(points2d, order, d_pts, r.choice).cpu().numpy()
    chosen = np.take_along_axis(pts, choice[..., None, None].astype(np.int64), axis=3)[:, :, :, 0]
    assert out.dtype == np.float64 and np.array_equal(out, og.relayout_19_to_38(chosen, order))
    moved = og.relayout_19_to_38(np.repeat((choice != 0)[..., None], 2, axis=-1).astype(np.float32), order)[..., 0] != 0
    assert np.array_equal((out != points2d.cpu().numpy()).any(axis=-1), moved)
    # entries that keep the input keep ITS bits, whatever they are: a marked input comes back where nothing moved
    marked = torch.full_like(points2d, -7.25)
    kept = ops.tracked_points2d(marked, order, d_pts, r.choice).cpu().numpy()
    assert np.all(kept[~moved] == -7.25) and np.array_equal(kept[moved], out[moved])


def test_without_a_motion_term_nothing_moves(native_lib, cuda):
    from deepfly3d_amd import ops

    count, pts, val, _ = tc.planted(seed=3, T=40, C=7, J=19)
    d_count, d_pts, d_val = _device((count, pts, val), cuda)
    r = ops.track_peaks(d_count, d_pts, d_val, IMAGE_SHAPE, w_motion=0.0)
    assert not r.choice.any() and not r.cost.any()
    points2d = ops.relayout_19_to_38(d_pts[:, :, :, 0].contiguous(), range(7))
    assert torch.equal(ops.tracked_points2d(points2d, range(7), d_pts, r.choice), points2d)
    assert ops.track_peaks(d_count, d_pts, d_val, IMAGE_SHAPE).choice.any()   # with it, the same input does move


def test_core_tracks_and_saves(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    """The two golden frames with the synthetic weights, through Core: the three keys follow points2d_argmax, points2d moved exactly where
    a chain left slot 0, and a save without tracking does not change by a byte."""
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    src, folder = os.path.join(golden_dir, "images"), tmp_path / "working"
    folder.mkdir()
    for f in os.listdir(src):
        os.symlink(os.path.join(src, f), folder / f)
    config.pop("image_shape", None)
    order = [0, 1, 2, 3, 4, 5, 6]
    core = Core(str(folder), str(tmp_path / "working_df3d"), num_images_max=2, camera_ordering=order)

    def saved_bytes():
        core.save()
        with open(core.save_path, "rb") as f:
            return f.read()

    core.pose2d_estimation(num_peaks=10)
    plain = saved_bytes()
    assert list(pickle.loads(plain)) == ["points2d", "camera_ordering", "heatmap_confidence"]
    argmax = core.points2d.copy()
    core.track_detections(w_value=0.05)   # two frames: a small value weight lets the jump decide
    saved = pickle.loads(saved_bytes())
    assert list(saved) == ["points2d", "camera_ordering", "heatmap_confidence", "points2d_argmax", "track_choice", "track_cost", "track_params"]
    want_choice, want_cost = to.solve(*core.peaks, tc.IMAGE_HW, 30.0, 1.0, 0.05)
    assert saved["track_choice"].dtype == np.int8 and np.array_equal(saved["track_choice"], want_choice)
    assert np.array_equal(saved["track_cost"], want_cost / 2.0 ** 20) and saved["track_params"].tolist() == [30.0, 1.0, 0.05]
    assert np.array_equal(saved["points2d_argmax"], argmax) and core._corrected
    moved = og.relayout_19_to_38(np.repeat((want_choice != 0)[..., None], 2, axis=-1).astype(np.float32), order)[..., 0] != 0
    print(f"chains off slot 0: {int((want_choice != 0).sum())} of {want_choice.size}; entries moved: {int(moved.sum())}")
    assert moved.any() and np.array_equal((saved["points2d"] != argmax).any(axis=-1), moved)
    chosen = np.take_along_axis(core.peaks[1], want_choice[..., None, None].astype(np.int64), axis=3)[:, :, :, 0]
    assert np.array_equal(saved["points2d"][moved], og.relayout_19_to_38(chosen, order)[moved])
    core.pose2d_estimation(num_peaks=10)   # forgets the tracking
    assert core._track is None and core.points2d_argmax is None and saved_bytes() == plain
    config.pop("image_shape", None)


def test_cli_track_2d(native_lib, cuda, tmp_path, golden_dir):
    """--track-2d through the command line: tracked before the first save, calibrated and triangulated from the tracked detections, the
    keys after the reference's."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, folder = os.path.join(golden_dir, "images"), tmp_path / "working"
    folder.mkdir()
    for f in os.listdir(src):
        os.symlink(os.path.join(src, f), folder / f)
    env = dict(os.environ, DF3D_SYNTHETIC_WEIGHTS="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-m", "deepfly3d_amd.cli", str(folder), "-n", "2", "--track-2d", "--track-value", "0.05", "--track-tau", "25"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = [f for f in os.listdir(str(folder) + "_df3d") if f.startswith("df3d_result")]
    assert len(files) == 1
    with open(os.path.join(str(folder) + "_df3d", files[0]), "rb") as f:
        res = pickle.load(f)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    assert [str(k) for k in res] == [str(k) for k in g3["key_order"]] + ["points2d_argmax", "track_choice", "track_cost", "track_params"]
    assert res["track_params"].tolist() == [25.0, 1.0, 0.05] and res["track_choice"].shape == (7, 2, 19) and res["track_choice"].any()
    moved = og.relayout_19_to_38(np.repeat((res["track_choice"] != 0)[..., None], 2, axis=-1).astype(np.float32), list(range(7)))[..., 0] != 0
    assert np.array_equal((res["points2d"] != res["points2d_argmax"]).any(axis=-1), moved)
    assert res["points3d_wo_procrustes"].shape == (2, 38, 3) and np.isfinite(res["points3d_wo_procrustes"]).all()
