"""CPU tests of the manual half of the correction workflow (reference df3d/core.py:253-284, 477-479, 509-544):
config.camera_see_joint / IGNORE_JOINT_ID against tables dumped from the reference (tests/golden/skeleton_tables.npz),
Core.nearest_joint, write_corrections, move_joint, save_corrections and check_cameras on the golden detections.  No GPU."""
import numpy as np
import pytest

HW = np.array([480.0, 960.0])   # (H, W): normalised -> pixels (row, col)


@pytest.fixture
def core(tmp_path, golden_dir):
    """A Core on the golden recording's detections and cameras with an empty correction store (no frames on disk are needed)."""
    from deepfly3d_amd.camera_network import CameraNetwork
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core
    from deepfly3d_amd.db import PoseDB

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    old = config.get("image_shape")
    config["image_shape"] = [960, 480]
    c = Core.__new__(Core)
    calib = {k: {"R": g3["R"][k], "tvec": g3["tvec"][k], "intr": g3["intr"][k], "distort": g3["distort"][k]} for k in range(7)}
    c.camNet = CameraNetwork(g3["points2d"] * HW, calib=calib, device="cpu")
    c.image_shape, c.num_images, c.max_img_id, c.is_primary, c.device = [960, 480], 15, 14, True, "cpu"
    c._output_folder = str(tmp_path)
    c.db = PoseDB(str(tmp_path))
    yield c
    if old is None:
        config.pop("image_shape", None)
    else:
        config["image_shape"] = old


def test_visibility_tables_equal_the_reference(golden_dir):
    from deepfly3d_amd import config as cfg

    t = np.load(f"{golden_dir}/skeleton_tables.npz")
    see = np.array([[cfg.camera_see_joint(c, j) for j in range(38)] for c in range(7)])
    assert see.dtype == bool and t["camera_see_joint"].shape == (7, 38) and np.array_equal(see, t["camera_see_joint"])
    assert cfg.IGNORE_JOINT_ID == [int(j) for j in t["ignore_joint_id"]]
    assert [cfg.camera_see_joint(7, j) for j in range(38)] == list(see[3])   # 7: the reference's alias of the front camera
    with pytest.raises(NotImplementedError):
        cfg.camera_see_joint(8, 0)


def test_visibility_is_consistent_with_the_relayout(golden_dir):
    """Every joint that the 19 -> 38 re-layout (df3d::relayout_source; its numpy restatement oracle.geometry.relayout_19_to_38)
    fills for a side camera is one the table says that camera sees; the only seen joints it leaves empty are the antennae of
    cameras 2 and 4, as the reference's own re-layout does (df3d/core.py:187-203)."""
    from oracle import geometry as og

    from deepfly3d_amd import config as cfg

    filled = og.relayout_19_to_38(np.full((7, 1, 19, 2), 0.5), list(range(7)))[:, 0, :, 0] != 0   # [7, 38], by the row coordinate (columns are un-flipped)
    see = np.array([[cfg.camera_see_joint(c, j) for j in range(38)] for c in range(7)])
    side = [0, 1, 2, 4, 5, 6]
    assert not (filled[side] & ~see[side]).any()
    assert [(int(c), int(j)) for c, j in np.argwhere(see & ~filled) if c != 3] == [(2, 15), (4, 34)]
    # the golden recording itself: no detection on a joint its camera cannot see
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    assert not ((g3["points2d"][..., 0] != 0) & ~see[:, None, :]).any()


def test_nearest_joint_sees_only_visible_joints_and_breaks_ties_low(core):
    from deepfly3d_amd.config import camera_see_joint

    rng = np.random.default_rng(3)
    for cam in range(7):
        seen = [j for j in range(38) if camera_see_joint(cam, j)]
        for _ in range(40):
            x, y = rng.uniform(0, 480), rng.uniform(0, 960)
            j = core.nearest_joint(cam, 4, x, y)
            assert isinstance(j, int) and j in seen
            pts = core.camNet.cam_list[cam][4]
            d = np.hypot(pts[seen, 0] - x, pts[seen, 1] - y)   # x against stored column 0 (rows), y against column 1 (columns)
            assert j == seen[int(np.argmin(d))]
    # the stored order: the exact pixel of a joint finds it, its transpose does not (a 480 x 960 image)
    r, c = core.camNet.cam_list[1][4][7]
    assert core.nearest_joint(1, 4, r, c) == 7 and core.nearest_joint(1, 4, c, r) != 7
    # ties go to the lowest id: two joints at one place, and a point midway between two joints
    core.camNet.points2d[1, 6, 3] = core.camNet.points2d[1, 6, 9] = [100.0, 200.0]
    assert core.nearest_joint(1, 6, 100.0, 200.0) == 3 and core.nearest_joint(1, 6, 101.0, 203.0) == 3
    core.camNet.points2d[1, 6, :19] = [[10.0 * j, 400.0] for j in range(19)]
    assert core.nearest_joint(1, 6, 45.0, 400.0) == 4 and core.nearest_joint(1, 6, 45.0 + 1e-9, 400.0) == 5
    # a stored correction is what the search looks at
    fix = core.camNet.cam_list[1][6].copy()
    fix[12] = [300.0, 700.0]
    core.db.write(fix / np.array([960.0, 480.0]), 1, 6, True, [12])
    assert core.nearest_joint(1, 6, 300.0, 700.0) == 12


def test_write_corrections_above_the_threshold_stores_the_pose(core):
    cam, img = 5, 3
    est = core.camNet.cam_list[cam][img].copy()
    pts = est.copy()
    pts[:] += 1.0          # every joint a little off, unseen ones (zeros in the estimate) included
    pts[22, 1] += 30.5     # joint 22 = femur-tibia of the first leg of camera 5's side: seen and checked
    core.write_corrections(cam, img, [22], pts)
    from deepfly3d_amd.config import camera_see_joint

    stored = core.db.read(cam, img)
    unseen = [j for j in range(38) if not camera_see_joint(cam, j)]
    seen = [j for j in range(38) if camera_see_joint(cam, j)]
    assert stored.shape == (38, 2) and not stored[unseen].any() and len(unseen) == 19
    assert np.array_equal(stored[seen], (pts / np.array([960, 480]))[seen])   # normalised by image_shape, as the reference divides
    assert core.db.db["train"][cam][img] is True and core.db.read_modified_joints(cam, img) == [22]
    assert core.db.last_write_image_id == img
    # what comes back is the pose in pixels
    back = core.corrected_points2d(cam, img)
    assert np.abs(back[seen] - pts[seen]).max() < 1e-9 and not back[unseen].any()
    assert np.array_equal(core.camNet.cam_list[cam][img], est)   # the estimate itself is untouched until corrected_points2d_matrix()


def test_write_corrections_below_the_threshold_removes_the_entry(core):
    cam, img = 5, 3
    est = core.camNet.cam_list[cam][img].copy()
    far = est.copy()
    far[22, 0] -= 31.0
    core.write_corrections(cam, img, [22], far)
    assert core.db.has_key(cam, img)
    near = est.copy()
    near[22] += [30.0, -30.0]       # exactly the threshold: not above it
    near[19] += 500.0               # body-coxa: seen, but on the ignore list
    near[34] += 500.0               # antenna: on the ignore list too
    near[3] += 500.0                # the other side: camera 5 cannot see it
    core.write_corrections(cam, img, [22], near)
    assert not core.db.has_key(cam, img) and core.db.read_modified_joints(cam, img) == [] and img not in core.db.db["train"][cam]
    core.write_corrections(cam, img, [], est)   # removing what is not there is fine
    assert not core.db.has_key(cam, img)


def test_move_joint_accumulates_sorted_unique_joints(core):
    cam, img = 1, 8
    est = core.camNet.cam_list[cam][img].copy()
    core.move_joint(cam, img, 8, est[8, 0] + 50.0, est[8, 1])
    assert core.db.read_modified_joints(cam, img) == [8]
    core.move_joint(cam, img, 3, est[3, 0], est[3, 1] - 70.0)
    core.move_joint(cam, img, 8, est[8, 0] + 60.0, est[8, 1])
    core.move_joint(cam, img, 13, est[13, 0] + 1.0, est[13, 1])
    assert core.db.read_modified_joints(cam, img) == [3, 8, 13]
    got = core.corrected_points2d(cam, img)
    want = est.copy()
    want[8, 0] += 60.0
    want[3, 1] -= 70.0
    want[13, 0] += 1.0
    assert np.abs(got - want).max() < 1e-9      # each move starts from the stored correction, not from the estimate
    # moving everything back home removes the entry, its joint list with it
    core.move_joint(cam, img, 8, *est[8])
    assert core.db.has_key(cam, img)
    core.move_joint(cam, img, 3, *est[3])
    assert not core.db.has_key(cam, img) and core.db.read_modified_joints(cam, img) == []


def test_save_corrections_round_trips_through_the_file(core, tmp_path):
    from deepfly3d_amd.db import PoseDB

    est = core.camNet.cam_list[0][2].copy()
    core.move_joint(0, 2, 7, est[7, 0] + 45.0, est[7, 1] + 45.0)
    core.move_joint(6, 11, 31, 200.0, 300.0)
    core.save_corrections()
    again = PoseDB(str(tmp_path))
    assert again.db_path == core.db.db_path
    for cam, img, joints in ((0, 2, [7]), (6, 11, [31])):
        assert again.has_key(cam, img) and again.read_modified_joints(cam, img) == joints and again.db["train"][cam][img] is True
        assert np.array_equal(again.read(cam, img), core.db.read(cam, img))
    assert np.abs(again.manual_corrections()[6][11][31] - [200.0, 300.0]).max() < 1e-9
    # corrected_points2d_matrix writes the stored poses into the camera network
    everything = core.corrected_points2d_matrix()
    assert everything is core.camNet.points2d and np.abs(everything[0, 2, 7] - (est[7] + 45.0)).max() < 1e-9


def test_check_cameras_names_an_emptied_camera(core):
    # the 19 -> 38 re-layout gives the front camera (ordering[3]) no detections, here as in the reference: it is always named
    with pytest.raises(AssertionError, match=r"Some cameras are missing: \[3\]"):
        core.check_cameras()
    core.camNet.cam_list[3].points2d[0, 15] = [240.0, 480.0]
    core.check_cameras()
    core.camNet.cam_list[2].points2d[:] = 0.0
    core.camNet.cam_list[5].points2d = None
    with pytest.raises(AssertionError, match=r"Some cameras are missing: \[2, 5\]"):
        core.check_cameras()


def test_smooth_points2d_needs_a_camera_network_and_rank_zero(core, monkeypatch):
    from deepfly3d_amd import distributed as dd

    net, core.camNet = core.camNet, None
    with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
        core.smooth_points2d(0)
    core.camNet = net
    monkeypatch.setattr(dd, "current", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="rank-0"):
        core.smooth_points2d(0)
    # the cache lives on the network and is dropped by the in-place writers
    net._smoothed = np.zeros((7, 15, 38, 2))
    monkeypatch.setattr(dd, "current", lambda: (0, 1))
    assert core.smooth_points2d(4) is not None and core.smooth_points2d(4).shape == (15, 38, 2)
    core.corrected_points2d_matrix()
    assert net._smoothed is None
