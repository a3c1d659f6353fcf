"""GPU tests of the kinematic chain behind Core.save's flags (deepfly3d_amd/kinematics.py): the all-flags
result of the 15-frame golden recording is pinned byte for byte to what the code before the chain wrote
(tests/golden/pose_chain_save_digests.json: one sha256 per key over dtype, shape and bytes, over the repr for the floats; recorded
twice, the two runs agreed), every other flag combination writes a sub-list of those keys with the same bytes, and one save runs
every stage once."""
import hashlib
import itertools
import json
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAGS = ("joint_angles", "rigid_legs", "angle_spectrogram", "behaviour_map")


def _expected_keys(joint_angles, rigid_legs, angle_spectrogram, behaviour_map):
    keys = ["joint_angles", "segment_lengths"] * joint_angles
    keys += ["points3d_rigid", "rigid_segment_lengths", "rigid_fit_cost"] * rigid_legs + ["joint_angles_rigid"] * (rigid_legs and joint_angles)
    keys += ["angle_spectrogram", "spectrogram_freqs", "spectrogram_fps"] * angle_spectrogram + ["angle_spectrogram_rigid"] * (angle_spectrogram and rigid_legs)
    keys += ["behaviour_map", "behaviour_map_train_index", "behaviour_map_kl", "behaviour_map_perplexity"] * behaviour_map
    return keys + ["behaviour_map_rigid", "behaviour_map_rigid_kl"] * (behaviour_map and rigid_legs)


def _digest(v):
    h = hashlib.sha256()
    if isinstance(v, np.ndarray):
        h.update(str(v.dtype).encode() + b"|" + repr(tuple(v.shape)).encode() + b"|" + np.ascontiguousarray(v).tobytes())
    else:
        h.update(repr(v).encode())
    return h.hexdigest()


class _Recording:
    """The recording test_core_* reopen (15 links to the sample's frame 0, an earlier result holding the golden detections and cameras),
    its Core, the keys of a plain save and the all-flags result."""

    def __init__(self, root, golden_dir):
        from deepfly3d_amd.config import config
        from deepfly3d_amd.core import Core

        folder = root / "working"
        folder.mkdir()
        for c in range(7):
            for t in range(15):
                os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
        folder = str(folder)
        g3 = np.load(f"{golden_dir}/golden_3d.npz")
        os.makedirs(folder + "_df3d")
        self.pkl = os.path.join(folder + "_df3d", "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
        res = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "distort": g3["distort"][c], "intr": g3["intr"][c]} for c in range(7)}
        res.update(points2d=g3["points2d"], camera_ordering=g3["camera_ordering"], heatmap_confidence=g3["heatmap_confidence"])
        with open(self.pkl, "wb") as f:
            pickle.dump(res, f)
        config.pop("image_shape", None)
        self.core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
        self.plain = list(self.save().keys())
        self.all = self.save(*FLAGS)

    def save(self, *flags):
        self.core.save(behaviour_perplexity=4, **{name: True for name in flags})
        with open(self.pkl, "rb") as f:
            return pickle.load(f)


@pytest.fixture(scope="module")
def recording(native_lib, cuda, tmp_path_factory, golden_dir):
    from deepfly3d_amd.config import config

    yield _Recording(tmp_path_factory.mktemp("pose_chain"), golden_dir)
    config.pop("image_shape", None)


def test_all_flags_result_is_the_pinned_one(recording, golden_dir):
    with open(os.path.join(golden_dir, "pose_chain_save_digests.json")) as f:
        pinned = json.load(f)
    assert list(pinned) == _expected_keys(True, True, True, True)
    assert list(recording.all.keys()) == recording.plain + list(pinned)   # the key order is part of the result
    got = {k: _digest(recording.all[k]) for k in pinned}
    assert got == pinned, [k for k in pinned if got[k] != pinned[k]]


@pytest.mark.parametrize("on", [c for c in itertools.product((False, True), repeat=4) if not all(c)], ids=lambda c: "".join("01"[b] for b in c))
def test_every_flag_combination_writes_the_same_bytes(recording, on):
    run = recording.save(*[name for name, flag in zip(FLAGS, on) if flag])
    assert list(run.keys()) == recording.plain + _expected_keys(*on)
    differ = [k for k in run if isinstance(k, str) and _digest(run[k]) != _digest(recording.all[k])]
    assert not differ, differ


def test_one_save_runs_each_stage_once(recording, monkeypatch):
    from deepfly3d_amd import ops

    calls = dict.fromkeys(("fit_legs", "recording_frame", "wavelet_spectrogram", "behaviour_map", "unwrap_phase", "joint_angles"), 0)

    def counted(name, fn):
        def wrapper(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)

        return wrapper

    for name in calls:
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
    recording.save(*FLAGS)
    print(calls)
    assert calls["fit_legs"] == 1 and calls["recording_frame"] == 1
    assert calls["wavelet_spectrogram"] == 2 and calls["behaviour_map"] == 2 and calls["unwrap_phase"] == 2
    assert calls["joint_angles"] <= 3   # measured, rigid, and the one inside segment_length_medians
    before = dict(calls)
    recording.core.joint_angles()   # the chain is not kept: a later call computes again
    assert calls["joint_angles"] > before["joint_angles"] and calls["recording_frame"] > before["recording_frame"]
