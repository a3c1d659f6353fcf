"""`Core`: the reference's orchestration surface (df3d.core.Core, reference df3d/core.py:62-544) on the
MI355X back-end.  Same constructor, methods, attributes, exceptions and result-pickle schema for the hot path:

    core = Core(input_folder, output_folder=None, num_images_max=None, camera_ordering=[0..6])
    core.pose2d_estimation(batch_size=8, disable_pin_memory=False)     # reference :170-203
    core.save()                                                        # reference :349-369
    core.calibrate_calc(min_img_id, max_img_id)                        # reference :229-250
    core.save()

The GUI itself is out of scope; the methods it drives are here: the correction store and
`corrected_points2d*`, through which stored corrections reach the triangulation, and the manual half of the correction workflow
(`nearest_joint`, `move_joint`, `write_corrections`, `check_cameras`, `smooth_points2d`).  The error navigation (`next_error`,
`prev_error`, `next_error_in_range`, `joint_has_error`, `get_joint_reprojection_error`) runs on the device.
"""
import dataclasses
import glob
import os
import pickle
import re
from typing import List, Optional

import numpy as np
import torch

from . import _native, logger, ops
from . import sync as sync_mod
from . import bundle_adjust as _ba
from . import config as config_mod
from .camera_network import CameraNetwork
from .config import IGNORE_JOINT_ID, SPECTROGRAM_FPS, camera_is_flipped, camera_see_joint, config, heatmap_planes, load_calibration, plane_color
from .db import PoseDB
from .inference import inference_folder
from .kinematics import PoseChain
from .os_util import camera_videos, extract_frames, get_max_img_id, image_path_for, parse_frame_rate, parse_vid_name, probe_frame_rate
from .procrustes import procrustes_separate, video_pose

_KNOWN_ORDERINGS = [
    (r"/CLC/", [0, 6, 5, 4, 3, 2, 1]),
    (r"/FA/", [6, 5, 4, 3, 2, 1, 0]),
    (r"/SG/", [6, 5, 4, 3, 2, 1, 0]),
    (r"Laura", [0, 6, 5, 4, 3, 2, 1]),
    (r"AYMANNS_Florian", [6, 5, 4, 3, 2, 1, 0]),
    (r"sample/test", [0, 1, 2, 3, 4, 5, 6]),
    (r"/JB/", [6, 5, 4, 3, 2, 1, 0]),
]


def find_default_camera_ordering(input_folder):
    """Lab-specific defaults keyed on the folder path (reference df3d/core.py:24-59)."""
    folder = str(input_folder)
    for pattern, order in _KNOWN_ORDERINGS:
        if re.search(pattern, folder):
            logger.debug(f"Default camera ordering found: {order}")
            return np.array(order)
    raise NotImplementedError(
        f"Cannot find camera ordering for folder {folder}. Please set your camera ordering using the --order flag. "
        "Example usage is df3d-cli /your/path/images/ --order 0 1 2 3 4 5 6"
    )


def relayout_points2d(points19, camera_ordering, device=None):
    """(7, T, 19, 2) network output -> (7, T, 38, 2) float64 skeleton layout, on the device
    (df3d_relayout_19_to_38; reference df3d/core.py:187-203)."""
    _native.require_gpu()
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    t = torch.as_tensor(np.ascontiguousarray(points19, dtype=np.float32)).to(dev)
    return ops.relayout_19_to_38(t, camera_ordering).cpu().numpy()


class Core:
    """Main interface to the 2-D and 3-D pose estimation (same surface as reference df3d/core.py:62)."""

    def __init__(self, input_folder: str, output_folder: Optional[str] = None, num_images_max: Optional[int] = None,
                 camera_ordering: List[int] = [0, 1, 2, 3, 4, 5, 6], dtype: str = "f32", device=None):
        from . import distributed as dd

        self.dtype, self.device = dtype, device
        rank, world = dd.current()
        self.is_primary = rank == 0  # multi-GPU: rank 0 alone expands videos, calibrates and writes results

        def everyone_waits():
            if world > 1:
                torch.distributed.barrier()

        self.input_folder = input_folder
        self.output_folder = output_folder if output_folder is not None else self.input_folder + "_df3d"
        if self.is_primary:
            self.expand_videos()
        everyone_waits()  # the frames exist for every rank from here on
        self.fps = self.get_fps()

        # frame range: ids 0 .. max_img_id, optionally cut to the first num_images_max
        self.num_images_max = num_images_max or 0
        last = get_max_img_id(self.input_folder)
        self.num_images = min(self.num_images_max, last + 1) if self.num_images_max > 0 else last + 1
        self.max_img_id = self.num_images - 1

        self._image_path = os.path.join(self.input_folder, "camera_{cam_id}_img_{img_id}.jpg")
        self.image_shape = self._resolve_image_shape(self._image_path.format(cam_id=0, img_id=0))

        if self.is_primary:
            self.db = PoseDB(self.output_folder)  # creates pose_corr_*.pkl on first use, like the reference
        everyone_waits()
        if not self.is_primary:
            self.db = PoseDB(self.output_folder)  # written by rank 0 above: loaded, not re-created
        self.camera_ordering = self.setup_camera_ordering(camera_ordering)
        self.camNet = self.points2d = self.points3d = self.conf = None
        self._points2d_shard = None  # multi-GPU: this rank's frames of points2d (device tensor, normalised), kept for the sharded DLT
        self.peaks = None             # (count, points, values) of pose2d_estimation(num_peaks=K), numpy [7, T, 19, ...]; rank 0
        self.points2d_argmax = None   # the arg-max detections, once auto_correct() has replaced points2d
        self._corrected = False       # every rank: auto_correct() or track_detections() ran (save() then triangulates on rank 0 alone)
        self._track = None            # rank 0: {choice, cost, params} of track_detections(), while points2d holds its result
        self._subpixel = False        # pose2d_estimation(subpixel=True) ran: save() appends the key "subpixel"
        self._heatmap_cache = None    # (img_id, luma [7, H, W], heat-maps [7, 19, 64, 128]) device tensors of the last heatmaps() call
        self._heatmap_proven = False  # a reduced-precision engine passed the canary on this recording's views (heatmaps())
        if os.path.exists(self.save_path):
            self._resume(self.save_path)

    @staticmethod
    def _resolve_image_shape(first_image):
        """[W, H] of the recording: read from the first frame, cross-checked with a configured shape, remembered in
        the config (reference df3d/core.py:84-100: same precedence, same ValueErrors)."""
        configured = config.get("image_shape")
        if os.path.exists(first_image):
            from PIL import Image

            with Image.open(first_image) as im:
                actual = list(im.size)
            if configured is not None and actual != configured:
                raise ValueError(f"Actual image shape {actual} does not match config.py image shape {configured}")
            config["image_shape"] = actual
            return actual
        if configured is None:
            raise ValueError(f"Image shape not specified in config and could not be read from {first_image}")
        return configured

    def _resume(self, result_file):
        """Re-open an earlier result: its poses and the cameras it holds (reference df3d/core.py:109-126)."""
        with open(result_file, "rb") as f:
            earlier = pickle.load(f)
        self.points2d, self.conf = earlier["points2d"], earlier["heatmap_confidence"]
        self.points3d = earlier.get("points3d", self.points3d)
        pixels = earlier["points2d"] * self.image_shape[::-1]
        self.camNet = CameraNetwork(pixels, calib=earlier, image_path=self._image_path, device=self.device)

    # -- properties -----------------------------------------------------------------------------------
    @staticmethod
    def _as_directory(path, create=False):
        if create:
            os.makedirs(path, exist_ok=True)
        path = os.path.abspath(path).rstrip("/")
        assert os.path.isdir(path), f"Not a directory {path}"
        return path

    @property
    def input_folder(self):
        return self._input_folder

    @input_folder.setter
    def input_folder(self, value):
        self._input_folder = self._as_directory(value)

    @property
    def output_folder(self):
        return self._output_folder

    @output_folder.setter
    def output_folder(self, value):
        self._output_folder = self._as_directory(value, create=True)

    @property
    def number_of_joints(self):
        return config["num_joints"]

    @property
    def has_pose(self):
        return True

    @property
    def has_calibration(self):
        return self.camNet.has_calibration()

    @property
    def save_path(self):
        flat = self.input_folder.replace("/", "_")
        return os.path.join(self.output_folder, f"df3d_result_{flat}.pkl")

    # -- hot path -------------------------------------------------------------------------------------
    def pose2d_estimation(self, batch_size: int = 8, disable_pin_memory: bool = False, num_peaks: int = 0, subpixel: bool = False):
        """2-D pose on every frame of every camera, then the 19 -> 38 joint layout (reference :170-203).

        Under `torch.distributed` (one process per GPU) every rank processes a contiguous range of frames and ONE
        gather brings the results to rank 0, which alone goes on to calibrate and save.
        `num_peaks=K` > 0 also keeps the K best local maxima of every heat-map in `self.peaks` for auto_correct().
        `subpixel=True` (opt-in) refines every detection, and every kept peak, inside its heat-map cell; save() then
        appends the key "subpixel" to the result."""
        from . import distributed as dd

        flip = [cam for idx, cam in enumerate(self.camera_ordering) if idx > 3]
        rank, world = dd.current()
        t0, t1 = dd.shard_range(self.num_images, world, rank)
        res = inference_folder(
            folder=self.input_folder, camera_ids_to_flip=flip, return_heatmap=False, return_confidence=True,
            max_img_id=self.max_img_id, batch_size=batch_size, disable_pin_memory=disable_pin_memory, dtype=self.dtype, device=self.device,
            frame_range=(t0, t1), as_device_tensors=True, return_peaks=num_peaks, subpixel=subpixel,
        )
        points19, conf, peaks = res[0], res[1], list(res[2:])
        # 19 -> 38 layout on the device, then (N > 1) ONE gather of the device tensors: no host round trip before it
        points2d = ops.relayout_19_to_38(points19.contiguous(), self.camera_ordering)
        self._points2d_shard = points2d if world > 1 else None
        self._corrected, self.points2d_argmax, self._track = False, None, None
        self._subpixel = bool(subpixel)
        if dd.collective_needed(world):
            gathered = dd.gather_packed([(points2d, 1), (conf, 1)] + [(p, 1) for p in peaks], self.num_images)
            self.is_primary = rank == 0
            if gathered is None:
                self.points2d = self.conf = self.peaks = None
                return
            points2d, conf, peaks = gathered[0], gathered[1], gathered[2:]
        self.points2d, self.conf = points2d.cpu().numpy(), conf.cpu().numpy()
        self.peaks = tuple(p.cpu().numpy() for p in peaks) if peaks else None

    def auto_correct(self, flagged_only=False, **params):
        """Pictorial-structures correction of the 2-D detections on the device: replaces `points2d` and the
        camera network's points by the corrected detections and keeps the arg-max ones in `points2d_argmax`.  Needs calibrated
        cameras (calibrate_calc) and the peaks of pose2d_estimation(num_peaks=K).  `params` override config.PICTORIAL_DEFAULTS
        (num_proposals, tau, w_reproj, w_heatmap, w_bone; num_peaks is fixed by the peaks kept).  `flagged_only=True` keeps the
        correction only on the joints that the reprojection-error test flags on the arg-max detections;
        every other detection stays the arg-max one, bit for bit.  Multi-GPU: every rank calls this, rank 0 solves, a failure
        there is raised on every rank (`distributed.agree`)."""
        from . import distributed as dd
        from .config import PICTORIAL_DEFAULTS

        error = None
        if self.is_primary:
            try:
                unknown = set(params) - set(PICTORIAL_DEFAULTS) - {"chunk_frames"}
                if unknown:
                    raise TypeError(f"auto_correct: unknown parameters {sorted(unknown)}")
                if self.camNet is None or not self.camNet.has_calibration():
                    raise RuntimeError("auto_correct needs calibrated cameras: run calibrate_calc() first")
                if self.peaks is None or self.points2d is None or self.peaks[0].shape[1] != self.points2d.shape[1]:
                    raise RuntimeError("auto_correct needs the heat-map peaks of this recording: run pose2d_estimation(num_peaks=K) first")
                self._auto_correct_primary(params, flagged_only)
            except Exception as e:  # noqa: BLE001  (re-raised by agree, on every rank)
                error = e
        dd.agree(error, "auto_correct")
        self._corrected = True

    def _auto_correct_primary(self, params, flagged_only=False):
        from .config import PICTORIAL_DEFAULTS

        p = {**PICTORIAL_DEFAULTS, **params}
        if "num_peaks" in params and int(params["num_peaks"]) != self.peaks[1].shape[3]:
            raise ValueError(f"num_peaks={params['num_peaks']}, but pose2d_estimation kept {self.peaks[1].shape[3]} peaks per heat-map")
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        count, pts, vals = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in self.peaks)
        argmax2d = self.points2d_argmax if self.points2d_argmax is not None else self.points2d
        am = torch.from_numpy(np.ascontiguousarray(argmax2d, dtype=np.float64)).to(dev)
        P = np.stack([c.P for c in self.camNet.cam_list])
        res = ops.pictorial_correct(P, self.camera_ordering, am, count, pts, vals, self.image_shape, num_proposals=p["num_proposals"], tau=p["tau"],
                                    w_reproj=p["w_reproj"], w_heatmap=p["w_heatmap"], w_bone=p["w_bone"], chunk_frames=p.get("chunk_frames", 4096))
        corrected, flagged = res.points2d, None
        if flagged_only:
            # the error test on the arg-max detections, at the point the correction starts from (its proposal 0); pixels = normalised
            # * (H, W), the product df3d_triangulate_scaled forms
            scale = torch.tensor([float(v) for v in self.image_shape[::-1]], dtype=torch.float64, device=dev)
            _, _, mask = ops.reprojection_errors(P, (am * scale).contiguous(), X=ops.arg_max_points3d(P, am, self.image_shape))
            bit = torch.ones((), dtype=torch.int64, device=dev) << torch.arange(am.shape[2], dtype=torch.int64, device=dev)
            flagged = (mask[:, None] & bit) != 0                                   # [T, 38]
            corrected = torch.where(flagged[None, :, :, None], res.points2d, am)
        self.points2d_argmax = np.array(argmax2d, dtype=np.float64, copy=True)
        self.points2d = corrected.cpu().numpy()
        self._track = None   # the correction started from the arg-max detections: an earlier tracking is gone
        np.copyto(self.camNet.points2d, self.points2d * self.image_shape[::-1])
        self.camNet.drop_smoothed()
        changed = int((self.points2d != self.points2d_argmax).any(axis=-1).sum())
        energy = f"mean minimum energy per frame {float(res.energy.mean()) if res.energy.numel() else 0.0:.4f}"
        if flagged is None:
            print(f"Auto-correction changed {changed} detections; {energy}")
        else:
            print(f"Auto-correction changed {changed} detections on {int(flagged.sum())} flagged joints; {energy}")

    def track_detections(self, **params):
        """Track the 2-D detections through time on the device: for every (camera, network joint) the sequence of
        heat-map peaks that is jointly best over the whole recording replaces the per-frame arg-max, in `points2d` and, when there is
        one, in the camera network's points; the arg-max detections are kept in `points2d_argmax`, and save() then writes
        "track_choice", "track_cost" and "track_params".  Needs the peaks of pose2d_estimation(num_peaks=K), no calibration.  It always
        starts from the arg-max detections, as auto_correct() does: of the two, the later call wins.  `params` override
        config.TRACK_DEFAULTS (tau, w_motion, w_value, block_frames); tau and the weights are guesses nobody has measured on a
        recording.  Multi-GPU: every rank calls this, rank 0 solves, a failure there is raised on every rank (`distributed.agree`)."""
        from . import distributed as dd
        from .config import TRACK_DEFAULTS

        error = None
        if self.is_primary:
            try:
                unknown = set(params) - set(TRACK_DEFAULTS)
                if unknown:
                    raise TypeError(f"track_detections: unknown parameters {sorted(unknown)}")
                p = ops.track_params(**params)   # refused before any device work
                if self.peaks is None or self.points2d is None or self.peaks[0].shape[1] != self.points2d.shape[1]:
                    raise RuntimeError("track_detections needs the heat-map peaks of this recording: run pose2d_estimation(num_peaks=K) first")
                self._track_primary(p)
            except Exception as e:  # noqa: BLE001  (re-raised by agree, on every rank)
                error = e
        dd.agree(error, "track_detections")
        self._corrected = True

    def _track_primary(self, p):
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        count, pts, vals = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in self.peaks)
        argmax2d = self.points2d_argmax if self.points2d_argmax is not None else self.points2d
        am = torch.from_numpy(np.ascontiguousarray(argmax2d, dtype=np.float64)).to(dev)
        res = ops.track_peaks(count, pts, vals, self.image_shape, *p)
        tracked = ops.tracked_points2d(am, self.camera_ordering, pts, res.choice)
        self.points2d_argmax = np.array(argmax2d, dtype=np.float64, copy=True)
        self.points2d = tracked.cpu().numpy()
        if self.camNet is not None and self.camNet.points2d is not None and self.camNet.points2d.shape == self.points2d.shape:
            np.copyto(self.camNet.points2d, self.points2d * self.image_shape[::-1])
            self.camNet.drop_smoothed()
        self._track = {"choice": res.choice.cpu().numpy().astype(np.int8), "cost": res.cost_float.cpu().numpy(),
                       "params": np.array(p[:3], dtype=np.float64)}
        moved = int((self._track["choice"] != 0).sum())
        print(f"Tracking moved {moved} of {self._track['choice'].size} detections off the arg-max peak; "
              f"mean cost per chain {float(self._track['cost'].mean()) if self._track['cost'].size else 0.0:.4f}")

    # -- suspect detections (reference df3d/core.py:205-227, 481-507) -----------------------------------------
    # Rank-0 methods on the camera network's detections (pixels, with auto-corrections and the manual corrections that
    # corrected_points2d_matrix() wrote into it), triangulated as save() triangulates them.  No cache: every call computes what it
    # needs, so an edit of the points never leaves stale flags.
    _ERROR_CHUNK_FIRST, _ERROR_CHUNK_LAST = 1024, 65536

    def _reprojection_on(self, ids):
        """(err [7, n, 38], jmax [n, 38], mask [n]) device tensors of the frames `ids` (host-gathered: a chunk, not the recording,
        travels to the device)."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError("the reprojection-error queries are rank-0 methods: the camera network lives on rank 0")
        if self.camNet is None or not self.camNet.has_calibration():
            raise RuntimeError("the reprojection-error queries need calibrated cameras: run calibrate_calc() first")
        px = self.camNet.points2d
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= px.shape[1]):
            raise IndexError(f"image ids must lie in [0, {px.shape[1]})")
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        P = np.stack([c.P for c in self.camNet.cam_list])
        return ops.reprojection_errors(P, torch.from_numpy(np.ascontiguousarray(px[:, ids])).to(dev))

    def reprojection_errors(self, frames=None):
        """Per-camera reprojection errors [7, nf, 38] in pixels of the frames `frames` (default all), as a numpy array."""
        if frames is None:
            frames = range(self.camNet.points2d.shape[1]) if self.camNet is not None else []
        return self._reprojection_on(frames)[0].cpu().numpy()

    def get_joint_reprojection_error(self, img_id, joint_id, camNet=None):
        """The largest reprojection error of joint `joint_id` on image `img_id` over the cameras, in pixels.  `camNet` (the
        reference's signature): the cameras to take the maximum over, camera ids or Camera objects (or a CameraNetwork)."""
        err, jmax, _ = self._reprojection_on([img_id])
        if camNet is None:
            return float(jmax[0, joint_id])
        cams = camNet.cam_list if hasattr(camNet, "cam_list") else camNet
        ids = [int(getattr(c, "cam_id", c)) for c in cams]
        return float(err[ids, 0, joint_id].max()) if ids else 0.0

    def joint_has_error(self, img_id, joint_id):
        """Whether joint `joint_id` of image `img_id` is flagged: its error exceeds config.REPROJ_THR[joint_id]."""
        mask = int(self._reprojection_on([img_id])[2][0])
        return bool((mask >> int(joint_id)) & 1)

    def next_error_in_range(self, range_of_ids):
        """The first image id of `range_of_ids`, in its order, with a flagged joint, or None.  Evaluated on the device in chunks of
        growing size (1 024 ids, doubling up to 65 536), stopping at the first chunk that holds a flagged frame."""
        import itertools

        it, size = iter(range_of_ids), self._ERROR_CHUNK_FIRST
        while True:
            ids = list(itertools.islice(it, size))
            if not ids:
                return None
            hit = torch.nonzero(self._reprojection_on(ids)[2]).flatten()
            if hit.numel():
                return ids[int(hit[0])]
            size = min(2 * size, self._ERROR_CHUNK_LAST)

    def next_error(self, img_id):
        """The next image after `img_id` with a flagged joint, or None (reference df3d/core.py:205-215)."""
        return self.next_error_in_range(range(img_id + 1, self.max_img_id + 1))

    def prev_error(self, img_id):
        """The previous image before `img_id` with a flagged joint, or None (reference df3d/core.py:217-227)."""
        return self.next_error_in_range(range(img_id - 1, -1, -1))

    # -- consensus triangulation: rank-0 methods on the detections save() triangulates, like the queries above ---
    def _robust_on(self, what, tau, min_views, ids=None, X=None):
        """(ops.ConsensusResult on the device, the pixel detections [7, n, 38, 2] it was computed from) of the frames `ids` (default
        all), with the refusals of _reprojection_on.  `tau`, `min_views`: ops.consensus_params' values.  `X`: the triangulation
        [T, 38, 3] of these very detections as a numpy array, where the caller has just computed it (save()); else it is computed here."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError(f"{what} is a rank-0 method: the camera network lives on rank 0")
        if self.camNet is None or not self.camNet.has_calibration():
            raise RuntimeError(f"{what} needs calibrated cameras: run calibrate_calc() first")
        px = self.camNet.points2d
        if ids is not None:
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
            if ids.size and (ids.min() < 0 or ids.max() >= px.shape[1]):
                raise IndexError(f"image ids must lie in [0, {px.shape[1]})")
            px = px[:, ids]
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        P = np.stack([c.P for c in self.camNet.cam_list])
        px = torch.from_numpy(np.ascontiguousarray(px, dtype=np.float64)).to(dev)
        if X is not None:
            X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
        return ops.triangulate_consensus(P, px, X, tau=tau, min_views=min_views), px

    def robust_triangulation(self, tau=None, min_views=None):
        """The consensus triangulation (ops.triangulate_consensus) of the camera network's detections -- the ones
        save() triangulates, stored corrections included -- an ops.ConsensusResult of numpy arrays: points3d [T, 38, 3] (in the layout
        of points3d_wo_procrustes), cameras [T, 38] int32 (bit c: camera c was used), status [T, 38] int8 (0 fewer than two views, 1
        all views agree, 2 a proper subset was chosen, 3 no subset qualified: the plain triangulation), error [7, T, 38] pixels (every
        view against the chosen point), fixed_px [7, T, 38, 2] (the detections with every rejected view replaced by the projection of
        the chosen point), counts [38, 4] and params (tau [38], min_views).  `tau`: pixels, one value or one per joint; the default,
        config.ROBUST_TAU, is a guess nobody has measured on a recording.  A rank-0 method with the refusals of the
        reprojection-error queries."""
        t, m = ops.consensus_params(tau, min_views)   # refused before any work
        r, _ = self._robust_on("robust_triangulation", t, m)
        return ops.ConsensusResult(*(v.cpu().numpy() for v in (r.points3d, r.cameras, r.status, r.error, r.fixed_px, r.counts)), r.params)

    def outlier_cameras(self, img_id, joint_id=None):
        """The cameras whose detection of joint `joint_id` on image `img_id` the consensus triangulation rejects (config.ROBUST_TAU,
        config.ROBUST_MIN_VIEWS), as a list of camera ids: the views to correct first.  `joint_id=None`: a dict joint id -> list, of
        the joints with a rejected view.  A rank-0 method with the refusals of the reprojection-error queries."""
        t, m = ops.consensus_params()
        r, px = self._robust_on("outlier_cameras", t, m, [img_id])
        view = (px[:, 0] != 0.0).all(dim=2).cpu().numpy()                        # [7, 38]
        used = (r.cameras[0].cpu().numpy()[None] >> np.arange(view.shape[0])[:, None]) & 1
        rejected = view & (used == 0) & (r.status[0].cpu().numpy() == 2)[None]
        if joint_id is not None:
            return [int(c) for c in np.nonzero(rejected[:, int(joint_id)])[0]]
        return {int(j): [int(c) for c in np.nonzero(rejected[:, j])[0]] for j in np.nonzero(rejected.any(axis=0))[0]}

    # -- camera frame lags: a rank-0 method on the detections save() triangulates ------------------------------------
    _SYNC_KEYS = ("sync_lag", "sync_status", "sync_pairs", "sync_pair_lag", "sync_pair_margin", "sync_pair_inconsistency", "sync_pair_cost",
                  "sync_pair_count", "sync_params")

    def _sync_on(self, what, params):
        """The sync.SyncResult on the device of the camera network's detections, with the refusals of _robust_on.  `params`:
        sync.sync_params' values."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError(f"{what} is a rank-0 method: the camera network lives on rank 0")
        if self.camNet is None or not self.camNet.has_calibration():
            raise RuntimeError(f"{what} needs calibrated cameras: run calibrate_calc() first")
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        P = np.stack([c.P for c in self.camNet.cam_list])
        px = torch.from_numpy(np.ascontiguousarray(self.camNet.points2d, dtype=np.float64)).to(dev)
        return sync_mod.camera_sync(P, px, *params)

    def camera_sync(self, **params):
        """The frame lag of every camera from the epipolar consistency of the camera network's detections -- the ones save()
        triangulates -- and the calibration (sync.camera_sync), a sync.SyncResult of numpy arrays: lag [7, nW]
        int32 (camera c shows instant t in its frame t + lag[c, t // window]), status [7] int8 (0 unobservable, 1 in step throughout, 2
        lagging somewhere), pairs, pair_lag, pair_margin, pair_inconsistency, pair_cost, pair_count, path_cost, F, points2d_px
        [7, T, 38, 2] (the detections with the lags undone, pixels) and params.  `params`: max_lag, window, tau, switch, min_count
        (sync.sync_params; the defaults are guesses nobody has measured on a recording).  Lags are relative within a group of cameras that
        share joints: one between the left and the right cameras cannot be seen.  A rank-0 method with the refusals of the
        reprojection-error queries."""
        r = self._sync_on("camera_sync", sync_mod.sync_params(**params))   # refused before any work
        return dataclasses.replace(r, **{f.name: getattr(r, f.name).cpu().numpy() for f in dataclasses.fields(r)
                                         if isinstance(getattr(r, f.name), torch.Tensor)})

    def _sync_keys(self, r):
        """The result keys of a SyncResult, in their order, and one log line per lagging camera."""
        host = lambda t: t.cpu().numpy()   # noqa: E731
        cost, count = host(r.pair_cost), host(r.pair_count)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = cost.astype(np.float64) / count.astype(np.float64) / float(config_mod.SYNC_COST_SCALE)
        window = r.params[1]
        for c in np.nonzero(r.status == 2)[0]:
            for w in range(r.lag.shape[1]):
                if r.lag[c, w] != (r.lag[c, w - 1] if w else 0):
                    logger.warning(f"camera {c} lags by {int(r.lag[c, w]):+d} frames from frame {w * window} on")
        return dict(zip(self._SYNC_KEYS, (r.lag, r.status, r.pairs, host(r.pair_lag), host(r.pair_margin), r.pair_inconsistency, mean, count,
                                          np.array(r.params, dtype=np.float64))))

    # -- trajectory triangulation: a rank-0 method on the detections save() triangulates ------------------------------
    def _trajectory_on(self, what, params, X=None, robust=None):
        """The ops.TrajectoryResult on the device of the camera network's detections, with the refusals of _robust_on.  `params`:
        ops.trajectory_params' values.  `X`: the triangulation [T, 38, 3] of these very detections as a numpy array where the caller
        has just computed it (save()); else it is computed here.  `robust`: None, or what _robust_on returned for these detections:
        the fit then starts from the robust points and sees only the views the consensus kept -- a rejected view is zeroed, not
        replaced by its projection, which would count the point's own projection as evidence."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError(f"{what} is a rank-0 method: the camera network lives on rank 0")
        if self.camNet is None or not self.camNet.has_calibration():
            raise RuntimeError(f"{what} needs calibrated cameras: run calibrate_calc() first")
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        P = np.stack([c.P for c in self.camNet.cam_list])
        if robust is not None:
            r, px = robust
            kept = ((r.cameras[None] >> torch.arange(px.shape[0], device=px.device)[:, None, None]) & 1) != 0
            kept |= (r.status == 0)[None]   # fewer than two views: the consensus rejected nothing there, and the lone view is evidence
            px, X = torch.where(kept[..., None], px, torch.zeros_like(px)), r.points3d
        else:
            px = torch.from_numpy(np.ascontiguousarray(self.camNet.points2d, dtype=np.float64)).to(dev)
            if X is not None:
                X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
        lam, huber, max_gap, _ = params
        return ops.triangulate_trajectory(P, px.contiguous(), X, lam=lam, huber=huber, max_gap=max_gap)

    def trajectory_triangulation(self, lam=None, huber=None, max_gap=None):
        """The trajectory triangulation (ops.triangulate_trajectory) of the camera network's detections -- the
        ones save() triangulates, stored corrections included -- an ops.TrajectoryResult of numpy arrays: points3d [T, 38, 3] (in the
        layout of points3d_wo_procrustes), status [T, 38] int8 (0 outside every segment: the plain triangulation's point, 1 anchor, 2
        a frame fewer than two cameras see, filled from its one view and its neighbours, 3 a frame no camera sees, 4 a frame of a joint
        whose fit did not converge), weight [7, T, 38] (below 1: the camera to correct), error [7, T, 38] pixels, iterations [38],
        cost [38, 2], counts [38, 5] and params (lam [38], huber, max_gap, block_frames).  `lam`: px^2 / mm^2, one value or one per
        joint; `huber`: pixels; both defaults (config.TRAJECTORY_LAMBDA, config.TRAJECTORY_HUBER) are guesses nobody has measured on
        a recording.  A rank-0 method with the refusals of the reprojection-error queries."""
        params = ops.trajectory_params(lam, huber, max_gap)   # refused before any work
        r = self._trajectory_on("trajectory_triangulation", params)
        return ops.TrajectoryResult(*(v.cpu().numpy() for v in (r.points3d, r.status, r.weight, r.error, r.iterations, r.cost, r.counts)),
                                    r.params)

    # -- heat-map triangulation: a rank-0 method on the images and the calibrated cameras ----------------------------
    def _heatmap3d_on(self, what, params, X=None, batch=16):
        """The heatmap3d.HeatmapTriangulation on the device of every frame of the camera network, with the refusals of _robust_on and
        of the heat-map queries.  `params`: heatmap3d_params' values.  `X`: the start points [T, 38, 3], a float64 device tensor or a
        numpy array (save()'s latest pose); None: the plain triangulation of the camera network's detections, computed here.  Batches of
        `batch` frames go through the file bytes, the device JPEG decode and the hourglass exactly as video._heatmap_frames sends them,
        one search launch per batch; the heat-maps of a batch (4.3 MB per frame) never reach the host and are dropped with it."""
        from . import distributed as dd
        from . import heatmap3d, jpeg
        from .inference import PREPROCESS, get_engine

        if dd.current()[0] != 0:
            raise RuntimeError(f"{what} is a rank-0 method: the camera network lives on rank 0")
        if self.camNet is None or not self.camNet.has_calibration():
            raise RuntimeError(f"{what} needs calibrated cameras: run calibrate_calc() first")
        if not self.has_heatmap:
            raise FileNotFoundError(f"{what} searches the heat-maps the network computes from the camera images, and {self.input_folder} "
                                    "holds none (deleted with --delete-images?): heat-maps are recomputed from the images, never stored")
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        cameras, flip, plane = heatmap3d.view_table(self.camera_ordering)
        P = np.stack([c.P for c in self.camNet.cam_list])
        if X is None:
            X = ops.triangulate(P, torch.from_numpy(np.ascontiguousarray(self.camNet.points2d, dtype=np.float64)).to(dev))
        elif not isinstance(X, torch.Tensor):
            X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
        T = int(X.shape[0])
        W, H = self.image_shape
        engine = get_engine(dtype=self.dtype, device=dev)
        flip_dev = torch.from_numpy(flip).to(dev)
        half, levels, floor = params

        def forward(e, luma, f):
            return e.forward_u8(luma, f, PREPROCESS["mean"], PREPROCESS["std"], resize=PREPROCESS["resize"])

        parts = []
        for t0 in range(0, T, batch):
            ids = range(t0, min(t0 + batch, T))
            blobs = []
            for i in ids:
                for cam in cameras:
                    with open(image_path_for(self.input_folder, int(cam), i), "rb") as f:
                        blobs.append(f.read())
            luma = jpeg.decode_luma(blobs, W, H, device=dev)   # [V n, H, W], image-major
            f = flip_dev.repeat(len(ids))
            V = len(cameras)
            if t0 == 0 and engine.dtype != "f32":   # a reduced-precision engine proves itself on the first image's views (HourglassEngine.canary)
                engine.canary(get_engine(dtype="f32", device=dev), lambda e: forward(e, luma[:V], f[:V]), what=f"the first views of {self.input_folder}")
            hm = forward(engine, luma, f)
            hm = hm.reshape(len(ids), V, *hm.shape[1:])
            parts.append(heatmap3d.triangulate_heatmaps(P[cameras], hm, flip, plane, X[t0:t0 + len(ids)].contiguous(), self.image_shape,
                                                        half=half, levels=levels, floor=floor))
            luma = hm = None
        if not parts:
            return heatmap3d.triangulate_heatmaps(P[cameras], torch.empty((0, len(cameras), config["num_predict"], 64, 128), dtype=torch.float32, device=dev),
                                                  flip, plane, X.contiguous(), self.image_shape, half=half, levels=levels, floor=floor)
        cat = lambda name: torch.cat([getattr(p, name) for p in parts])   # noqa: E731
        return heatmap3d.HeatmapTriangulation(cat("points3d"), cat("score"), cat("status"), cat("views"), cat("shift"), cat("choice"),
                                              torch.stack([p.counts for p in parts]).sum(dim=0), parts[0].params, cat("path"))

    def heatmap_triangulation(self, half=None, levels=None, floor=None):
        """The heat-map triangulation (heatmap3d.triangulate_heatmaps) of every frame, a
        heatmap3d.HeatmapTriangulation of numpy arrays: points3d [T, 38, 3] (in the layout of points3d_wo_procrustes), score [T, 38]
        (NaN where nothing was searched), status [T, 38] int8 (0 fewer than two views or no start point: the plain triangulation's
        point, 1 searched, 2 no evidence within the cube: the plain triangulation's point, 3 searched, and the best point of the first
        level lay on a face of the cube), views [T, 38] int32 (bit v: the v-th camera that has planes, in ascending camera id), shift
        [T, 38] mm, choice [T, 38, levels], counts [38, 4] and params (half, levels, floor, grid).  The search starts at the plain
        triangulation of the camera network's detections and reads the heat-maps the network computes from the images, on the run's
        own path (Core.heatmaps); they are never stored, so the images must be present.  `half` (mm), `levels` and `floor` default to
        config.HEATMAP3D_*, guesses nobody has measured on a recording.  A rank-0 method with the refusals of the reprojection-error
        queries."""
        from . import heatmap3d

        params = heatmap3d.heatmap3d_params(half, levels, floor)   # refused before any work
        r = self._heatmap3d_on("heatmap_triangulation", params)
        return heatmap3d.HeatmapTriangulation(*(v.cpu().numpy() for v in (r.points3d, r.score, r.status, r.views, r.shift, r.choice, r.counts)),
                                              r.params, r.path.cpu().numpy())

    # -- the kinematic chain (DESIGN.md sections 14-17): one kinematics.PoseChain per call, never kept ----------------------------------
    def _measured_pose(self, what, fps=None, repair=None, pose=None):
        """The PoseChain of camNet.points3d on the device (triangulating first when there is none), with the refusals of the rank-0
        pose queries.  `repair`: None or False, or the chain of the repaired pose instead: True for the default
        parameters, or a dict of ops.repair_pose's.  `pose`: a [T, 38, 3] float64 device tensor to build the chain from in place of
        camNet.points3d (save()'s robust pose)."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError(f"{what} is a rank-0 method: the camera network lives on rank 0")
        if self.camNet is None or not self.camNet.has_calibration():
            raise RuntimeError(f"{what} needs calibrated cameras: run calibrate_calc() first")
        if pose is None and self.camNet.points3d is None:
            self.camNet.triangulate()
        _native.require_gpu()
        dev = torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")
        chain = PoseChain(torch.from_numpy(np.ascontiguousarray(self.camNet.points3d, dtype=np.float64)).to(dev) if pose is None else pose, fps)
        return chain.repaired(**(repair if isinstance(repair, dict) else {})) if repair else chain

    def repair_pose(self, half_window=None, threshold=None, floor=None, max_gap=None, min_count=None):
        """The repaired pose (ops.repair_pose) of the triangulation `camNet.points3d`, an ops.PoseRepairResult of
        numpy arrays: points [T, 38, 3] (outliers and missing joints interpolated linearly over gaps of at most `max_gap` frames, set
        to 0 -- missing -- where the gap is longer or touches an end of the recording), status [T, 38] int8 (0 kept, 1 missing and
        filled, 2 outlier and filled, 3 missing and left, 4 outlier and removed), counts [38, 5], score [T, 38] (the Hampel test's
        largest deviation / bound; NaN for a missing or untested joint) and params (half_window, threshold, floor, max_gap,
        min_count).  The defaults, config.REPAIR_*, are guesses nobody has measured on a recording.  Triangulates first when there
        is no points3d yet.  A rank-0 method with joint_angles' refusals."""
        params = dict(zip(("half_window", "threshold", "floor", "max_gap", "min_count"),
                          ops.repair_params(half_window, threshold, floor, max_gap, min_count)))   # refused before any work
        r = self._measured_pose("repair_pose", repair=params).repair
        return ops.PoseRepairResult(r.points.cpu().numpy(), r.status.cpu().numpy(), r.counts.cpu().numpy(), r.score.cpu().numpy(), r.params)

    def joint_angles(self, body_frame="recording", rigid=False, repair=False):
        """(angles [T, 6, 8] radians, lengths [T, 6, 4]) as numpy arrays: the eight joint angles (config.LEG_ANGLE_NAMES) and four
        segment lengths of every leg (config.LEG_NAMES), ops.joint_angles of the triangulation `camNet.points3d` -- what the result
        calls points3d_wo_procrustes; the per-side Procrustes result registers the two sides separately and is not the input.
        Triangulates first when the camera network holds no points3d yet; after editing detections call camNet.triangulate() (save()
        does).  `body_frame`: "recording" (default), "per_frame" or an explicit [3, 3] / [T, 3, 3] array.  `rigid=True`: the angles of
        the constant-length pose rigid_legs() fits, whose lengths are the fixed ones; "recording" is then still
        the recording frame of the MEASURED pose, so that both sets of angles share one frame.  `repair=True`: of the repaired pose
        (repair_pose() with its defaults), whose recording frame is its own.  A rank-0 method, like the
        reprojection-error queries."""
        chain = self._measured_pose("joint_angles", repair=repair)
        angles, lengths = (chain.rigid() if rigid else chain).joint_angles(body_frame)
        return angles.cpu().numpy(), lengths.cpu().numpy()

    def rigid_legs(self, lengths="recording", anchor="per_frame", repair=False):
        """(points [T, 38, 3], lengths [6, 4], cost [T, 6]) as numpy arrays: the triangulation `camNet.points3d` with every leg replaced
        by the chain of constant segment lengths that lies closest to its measured joints (ops.fit_legs), the lengths used, and each
        leg's summed squared distance from the measured joints (NaN where a leg misses a joint and is left as measured).  `lengths`:
        "recording" (every segment's median over the recording) or a [6, 4] array; `anchor`: "per_frame", "recording" or a [6, 3]
        array.  `repair=True`: the fit of the repaired pose (repair_pose() with its defaults).  Triangulates first when there is no
        points3d yet.  A rank-0 method with joint_angles' refusals."""
        fit = ops.fit_legs(self._measured_pose("rigid_legs", repair=repair).points3d, lengths, anchor)
        return fit.points.cpu().numpy(), np.array(fit.lengths), fit.cost.cpu().numpy()

    def _wavelet_bank(self, what, fps, bank):
        """(fps, {freqs, omega0, radius}) of angle_spectrogram's `fps` and `bank`, refused before any device work."""
        unknown = set(bank) - {"f_min", "f_max", "num", "freqs", "omega0", "radius"}
        if unknown:
            raise TypeError(f"{what} got unexpected bank arguments {sorted(unknown)}")
        if "freqs" in bank and {"f_min", "f_max", "num"} & set(bank):
            raise TypeError("give either freqs or f_min / f_max / num, not both")
        if fps is None:
            fps = self.get_fps()
        if fps is None:
            fps = SPECTROGRAM_FPS
        fps = float(fps)
        freqs = bank["freqs"] if "freqs" in bank else ops.wavelet_frequencies(fps, bank.get("f_min"), bank.get("f_max"), bank.get("num"))
        return fps, dict(freqs=np.ascontiguousarray(freqs, dtype=np.float64), omega0=bank.get("omega0"), radius=bank.get("radius"))

    def angle_spectrogram(self, rigid=False, body_frame="recording", fps=None, unwrap=True, repair=False, **bank):
        """(S [T, 6, 8, F], freqs [F]) as numpy arrays: the Morlet wavelet amplitudes (ops.wavelet_spectrogram, radians) of the
        48 joint-angle series joint_angles(body_frame, rigid) returns, and the rows' frequencies in Hz.  `fps`: the sampling rate;
        None means get_fps(), and where that is None config.SPECTROGRAM_FPS.  `unwrap=True` first applies numpy.unwrap's rule
        along time to the angles that live on the full circle (config.SPECTROGRAM_UNWRAPPED_ANGLES): a wrap at +-pi is otherwise
        a step of 2 pi that lights up every row.  A series that holds a non-finite sample is left wrapped and named in one logged
        warning.  `bank`: f_min, f_max, num (ops.wavelet_frequencies) or freqs, and omega0, radius.  `repair=True`: of the repaired
        pose (repair_pose() with its defaults).  A rank-0 method with joint_angles' refusals."""
        fps, bank = self._wavelet_bank("angle_spectrogram", fps, bank)
        chain = self._measured_pose("angle_spectrogram", fps, repair)
        return (chain.rigid() if rigid else chain).spectrogram(body_frame, unwrap, **bank).cpu().numpy(), bank["freqs"]

    def behaviour_map(self, rigid=False, perplexity=None, n_iter=None, max_points=None, seed=0, repair=False, **spectrogram_kwargs):
        """The behaviour map (ops.behaviour_map) of the float64 spectrogram angle_spectrogram(rigid, **spectrogram_kwargs) computes,
        every frame's [6, 8, F] amplitudes flattened to one spectrum: an ops.BehaviourMapResult of numpy arrays -- embedding [T, 2]
        (NaN for a frame whose spectrum holds a NaN), train_index [N], beta [T], info [T], kl and perplexity.  A recording too
        short for the perplexity (3 perplexity <= frames - 1) is refused before anything is computed.  `repair=True`: of the repaired
        pose (repair_pose() with its defaults).  A rank-0 method with angle_spectrogram's refusals."""
        bank = dict(spectrogram_kwargs)
        body_frame, fps, unwrap = bank.pop("body_frame", "recording"), bank.pop("fps", None), bank.pop("unwrap", True)
        frames = getattr(self, "num_images", None)
        if frames is not None and self.camNet is not None and self.camNet.has_calibration():
            ops.behaviour_map_points(frames, perplexity, max_points)   # before any work
        fps, bank = self._wavelet_bank("behaviour_map", fps, bank)
        chain = self._measured_pose("behaviour_map", fps, repair)
        r = (chain.rigid() if rigid else chain).behaviour_map(perplexity, n_iter, max_points, seed, body_frame=body_frame, unwrap=unwrap, **bank)
        return ops.BehaviourMapResult(r.embedding.cpu().numpy(), r.train_index.cpu().numpy(), r.beta.cpu().numpy(), r.info.cpu().numpy(), r.kl,
                                      r.perplexity)

    def behaviour_segments(self, rigid=False, grid=None, sigma=None, min_peak=None, repair=False, **behaviour_map_kwargs):
        """The segmentation (ops.segment_map) of the map behaviour_map(rigid, **behaviour_map_kwargs) computes, the map itself
        computed once: an ops.BehaviourSegmentsResult of numpy arrays -- density [G, G], origin (x0, y0, h), sigma, regions [G, G]
        int32, region_peaks [R, 2], labels [T] int32 (-1 for a frame without a place on the map, 0 for one outside every region),
        bouts [B, 3] int64 (label, start, length), occupancy [R + 1] and transitions [R + 1, R + 1] int64.  `grid`, `sigma`,
        `min_peak`: config.BEHAVIOUR_GRID, config.BEHAVIOUR_DENSITY_SIGMA_FRACTION of the map's extent and
        config.BEHAVIOUR_MIN_PEAK by default.  `repair=True`: of the repaired pose (repair_pose() with its defaults).  A rank-0 method
        with behaviour_map's refusals."""
        kw = dict(behaviour_map_kwargs)
        perplexity, max_points = kw.pop("perplexity", None), kw.pop("max_points", None)
        n_iter, seed = kw.pop("n_iter", None), kw.pop("seed", 0)
        body_frame, fps, unwrap = kw.pop("body_frame", "recording"), kw.pop("fps", None), kw.pop("unwrap", True)
        frames = getattr(self, "num_images", None)
        if frames is not None and self.camNet is not None and self.camNet.has_calibration():
            ops.behaviour_map_points(frames, perplexity, max_points)   # before any work
        fps, bank = self._wavelet_bank("behaviour_segments", fps, kw)
        chain = self._measured_pose("behaviour_segments", fps, repair)
        _, s = (chain.rigid() if rigid else chain).behaviour_segments(grid, sigma, min_peak, perplexity=perplexity, n_iter=n_iter,
                                                                      max_points=max_points, seed=seed, body_frame=body_frame, unwrap=unwrap, **bank)
        return ops.BehaviourSegmentsResult(*(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in s))

    _GAIT_KEYS = ("gait_tip_position", "gait_tip_velocity", "gait_states", "gait_steps", "gait_step_metrics", "gait_phase", "gait_coupling",
                  "gait_coupling_count", "gait_pattern", "gait_pattern_histogram", "gait_state_counts", "gait_thresholds", "gait_fps")

    def _gait_fps(self, fps):
        """angle_spectrogram's rule: `fps`, else get_fps(), else config.SPECTROGRAM_FPS."""
        if fps is None:
            fps = self.get_fps()
        return float(SPECTROGRAM_FPS if fps is None else fps)

    def gait(self, rigid=False, fps=None, on=None, off=None, half_window=None, repair=False):
        """The gait analysis (ops.gait) of the triangulation `camNet.points3d` in the recording's body frame, an
        ops.GaitResult of numpy arrays: tip and vel [T, 6, 3] (every leg's tip relative to its body-coxa joint and its velocity, in
        leg coordinates), states [T, 6] int32 (-1 unknown, 0 stance, 1 swing), steps [S, 4] int64 (leg, lift-off, touch-down, next
        lift-off) and step_metrics [S, 3] (swing duration, stance duration, stride), phase [T, 6], coupling [6, 6, 2] and
        coupling_count [6, 6], pattern [T] int32 (the mask of the legs in swing; config.GAIT_TRIPODS), pattern_histogram [64],
        state_counts [6, 3], thresholds (on, off, half_window) and fps.  `fps`: None means get_fps(), and where that is None
        config.SPECTROGRAM_FPS.  `on`, `off`: the swing thresholds on the tip's anterior velocity, config.GAIT_SWING_ON and
        GAIT_SWING_OFF by default -- a guess nobody has measured on a recording; `half_window`: config.GAIT_DIFF_HALF.  `rigid=True`:
        of the constant-length pose rigid_legs() fits, in the recording frame of the measured pose.  `repair=True`: of the repaired
        pose (repair_pose() with its defaults).  A rank-0 method with joint_angles' refusals."""
        thresholds = dict(zip(("on", "off", "half_window"), ops.gait_thresholds(on, off, half_window)))   # refused before any work
        chain = self._measured_pose("gait", ops._gait_fps(self._gait_fps(fps)), repair)
        g = (chain.rigid() if rigid else chain).gait(**thresholds)
        values = (getattr(g, f.name) for f in dataclasses.fields(g))
        return ops.GaitResult(*(v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in values))

    @staticmethod
    def _gait_values(g):
        """The values of _GAIT_KEYS from a GaitResult of device tensors."""
        host = lambda t: t.cpu().numpy()   # noqa: E731
        return (host(g.tip), host(g.vel), host(g.states).astype(np.int8), host(g.steps), host(g.step_metrics), host(g.phase), host(g.coupling),
                host(g.coupling_count), host(g.pattern), host(g.pattern_histogram), host(g.state_counts), np.array(g.thresholds, dtype=np.float64),
                g.fps)

    _TREADMILL_KEYS = ("treadmill_ball_center", "treadmill_ball_radius", "treadmill_ball_rms", "treadmill_ball_count", "treadmill_ball_status",
                       "treadmill_rotation", "treadmill_legs", "treadmill_residual", "treadmill_fictive", "treadmill_path", "treadmill_skipped",
                       "treadmill_params", "treadmill_fps")

    def treadmill(self, fps=None, radius=None, on=None, off=None, half_window=None, min_legs=None, repair=False):
        """The treadmill ball and the fictive walking path (ops.treadmill) of the triangulation `camNet.points3d`
        in the recording's body frame, an ops.TreadmillResult of numpy arrays: tip and vel [T, 6, 3] (every leg's tip relative to the
        mean of the coxa medians and its velocity, in body coordinates), states [T, 6] int32, ball (an ops.BallFit: center [3], radius,
        rms, count, status -- bit 0: the fit was refused and everything after it is NaN), rotation [T, 3] (the ball's rotation
        vector, rad/s), legs [T] int32 (the stance legs it was fitted to), residual [T], fictive [T, 3] (forward and sideways speed
        in pose units (mm) per second, yaw rate in rad/s), path [T, 3] (x, y, theta), skipped (the frames that moved nothing), params
        (radius or NaN, on, off, half_window, min_legs, iterations) and fps.  `radius`: the ball's known radius in mm; None fits it,
        and noise biases the fitted radius low.  `fps`, `on`, `off`, `half_window`: gait()'s; `min_legs`: config.BALL_MIN_LEGS.  Every
        default is a guess nobody has measured on a recording.  `repair=True`: of the repaired pose (repair_pose() with its
        defaults), which is what a spiked tip asks for.  A rank-0 method with joint_angles' refusals."""
        params = dict(zip(("radius", "min_legs"), ops.treadmill_params(radius, min_legs)))   # refused before any work
        params.update(zip(("on", "off", "half_window"), ops.gait_thresholds(on, off, half_window)))
        chain = self._measured_pose("treadmill", ops._gait_fps(self._gait_fps(fps)), repair)
        r = chain.treadmill(**params)
        host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v   # noqa: E731
        values = {f.name: host(getattr(r, f.name)) for f in dataclasses.fields(r)}
        values["ball"] = ops.BallFit(host(r.ball.ball), host(r.ball.info), host(r.ball.sums))
        values["skipped"] = int(values["skipped"])
        return ops.TreadmillResult(**values)

    @staticmethod
    def _treadmill_values(r, thresholds=None):
        """The values of _TREADMILL_KEYS from a TreadmillResult of device tensors.  `thresholds`: the (on, off) behind states that were
        handed in, for the stored parameters."""
        host = lambda t: t.cpu().numpy()   # noqa: E731
        ball, info = host(r.ball.ball), host(r.ball.info)
        if thresholds is not None:
            r = dataclasses.replace(r, params=(r.params[0], *thresholds, *r.params[3:]))
        return (ball[:3].copy(), float(ball[3]), float(ball[4]), int(info[0]), int(info[1]), host(r.rotation), host(r.legs), host(r.residual),
                host(r.fictive), host(r.path), int(r.skipped.item()), np.array(r.params, dtype=np.float64), r.fps)

    # -- manual corrections (reference df3d/core.py:253-296, 477-479, 509-544) ---------------------------------
    _MOVE_THRESHOLD = 30   # pixels, per coordinate: a pose that differs less from the estimate on every checked joint is not stored

    def nearest_joint(self, cam_id, img_id, x, y):
        """The id of the joint of image `img_id` of camera `cam_id` that lies nearest to (x, y), among the joints the camera can
        see (config.camera_see_joint; the others are put at (9999, 9999) first, as in the reference), in
        corrected_points2d(cam_id, img_id).  Argument order and comparison are the reference's: `x` is compared with stored
        column 0 and `y` with stored column 1, and the stored columns are (row_px, col_px) -- so `x` is the ROW and `y` the COLUMN
        of the pixel.  Euclidean distance, ties to the lowest id; plain numpy.  (A point more than ~4 000 px from every seen joint
        is nearer to (9999, 9999); inside an image that cannot happen.)"""
        pts = self.corrected_points2d(cam_id, img_id)
        pts[[j for j in range(len(pts)) if not camera_see_joint(cam_id, j)]] = [9999, 9999]
        return int(np.argmin(np.hypot(pts[:, 0] - x, pts[:, 1] - y)))

    def move_joint(self, cam_id, img_id, joint_id, x, y):
        """Move joint `joint_id` of one image to (x, y) = (row_px, col_px), the stored order (see nearest_joint), and store the
        pose as a manual correction through write_corrections (reference df3d/core.py:277-284)."""
        modified = sorted(set(list(self.db.read_modified_joints(cam_id, img_id)) + [int(joint_id)]))
        points = self.corrected_points2d(cam_id, img_id)
        points[joint_id] = np.array([x, y])
        self.write_corrections(cam_id, img_id, modified, points)

    def write_corrections(self, cam_id, img_id, modified_joints, points2d):
        """Store `points2d` [38, 2] pixels (row, col), ALL joints of the image, as its manual correction -- if it differs from the
        camera network's estimate by more than 30 px in a coordinate of a joint the camera sees and config.IGNORE_JOINT_ID does not
        list; unseen joints are stored as zero, the pose normalised by `image_shape` and marked for training.  A pose nearer than
        that removes the stored correction (reference df3d/core.py:509-544).  save_corrections() writes the store to disk."""
        joints = range(config["num_joints"])
        seen = [j for j in joints if camera_see_joint(cam_id, j)]
        checked = [j for j in seen if j not in IGNORE_JOINT_ID]
        points2d = np.asarray(points2d, dtype=np.float64)
        if np.any(np.abs(self.camNet.cam_list[cam_id][img_id] - points2d)[checked] > self._MOVE_THRESHOLD):
            stored = points2d.copy()
            stored[[j for j in joints if j not in seen], :] = 0.0
            # (the reference divides (row, col) by image_shape = [W, H] as it stands; manual_corrections() multiplies by the same)
            self.db.write(stored / self.image_shape, cam_id, img_id, True, list(modified_joints))
        else:
            self.db.remove_corrections(cam_id, img_id)

    def check_cameras(self):
        """AssertionError naming the cameras without a single detection (reference df3d/core.py:477-479).  The 19 -> 38 re-layout
        gives the front camera (ordering[3]) none, here as in the reference, so a recording straight from pose2d_estimation names it."""
        cam_missing = [cam.cam_id for cam in self.camNet.cam_list if cam.is_empty()]
        assert not cam_missing, "Some cameras are missing: {}".format(cam_missing)

    def smooth_points2d(self, cam_id, refresh=False):
        """[T, 38, 2] pixels: the detections of camera `cam_id` smoothed along time for display (reference df3d/core.py:286-296;
        DESIGN.md section 11).  All cameras are smoothed in one launch on the first call and kept on the camera network; a new
        network (calibrate_calc, reopening a result), auto_correct() and corrected_points2d_matrix() drop them, `refresh=True`
        recomputes.  The result is a read-only view of the kept array: copy it before editing.  The reference keeps its cache in a mutable default argument, `private_cache=dict()`, which every Core of the
        process shares, so that a second recording gets the first one's points: that is a bug and not reproduced.  A rank-0 method,
        like the reprojection-error queries."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError("smooth_points2d is a rank-0 method: the camera network lives on rank 0")
        if self.camNet is None:
            raise RuntimeError("smooth_points2d needs the camera network: run calibrate_calc() first")
        return self.camNet.smooth_points2d(refresh=refresh)[cam_id]

    def calibrate_calc(self, min_img_id, max_img_id, loss=None, f_scale=None):
        """Bundle adjustment from the shipped initial calibration (reference :229-250; like the reference the
        image-id range is accepted and unused).  Multi-GPU: rank 0 solves, EVERY rank calls this and leaves it together --
        a failure on rank 0 (the solver, the disk) is raised on all ranks (`distributed.agree`).
        `loss`, `f_scale` (defaults config.BA_LOSS = 'linear', config.BA_F_SCALE pixels): a robust loss on the reprojection residuals,
        scipy's least_squares(loss=, f_scale=) per scalar residual -- 'soft_l1' is the one to use; a wrong
        detection then stops pulling the cameras.  With a loss other than 'linear', save() appends, after every other key, "ba_weight"
        [7, T, 38] float64 (the smaller rho' of the detection's two residuals: 1 where it took part at full weight, NaN where it was
        not in the adjustment), "ba_counts" [7, 3] (per camera: observations, those with weight below 0.5, the mean weight) and
        "ba_params" (loss, f_scale); calibration_outliers() lists the detections the calibration disbelieved.  'linear' changes
        nothing: the reference's sum of squares, and the result's schema as it was."""
        from . import distributed as dd

        loss = config_mod.BA_LOSS if loss is None else loss
        f_scale = config_mod.BA_F_SCALE if f_scale is None else f_scale
        _ba.loss_code(loss, f_scale)    # refused before any work, on every rank
        error = None
        self._ba_robust = None
        if self.is_primary:
            try:
                calib = load_calibration()
                reordered = {int(cidx): calib[idx] for idx, cidx in enumerate(self.camera_ordering)}
                self.camNet = CameraNetwork(self.points2d * self.image_shape[::-1], calib=reordered, image_path=self._image_path, device=self.device)
                if loss == "linear":
                    self.camNet.bundle_adjust(update_intrinsic=False, update_distort=False)
                else:
                    info = self.camNet.bundle_adjust(update_intrinsic=False, update_distort=False, loss=loss, f_scale=float(f_scale))
                    self._ba_robust = self._ba_robust_keys(info, loss, float(f_scale))
                print(f"Reprojection error is {self.camNet.reprojection_error()}")
            except Exception as e:  # noqa: BLE001  (re-raised by agree, on every rank)
                error = e
        dd.agree(error, "calibrate_calc")

    def _ba_robust_keys(self, info, loss, f_scale):
        """The result keys of a robust calibration, from the camera network's solver info."""
        T, stride = self.camNet.points2d.shape[1], int(info["frame_stride"])
        weight = np.full(self.camNet.points2d.shape[:3], np.nan, dtype=np.float64)
        weight[:, ::stride][:, : info["obs_weight"].shape[1]] = info["obs_weight"]   # (a recording above ba_max_images: the strided frames)
        seen = ~np.isnan(weight)
        with np.errstate(invalid="ignore"):
            low = seen & (weight < 0.5)
        counts = np.zeros((weight.shape[0], 3), dtype=np.float64)
        counts[:, 0], counts[:, 1] = seen.sum(axis=(1, 2)), low.sum(axis=(1, 2))
        counts[:, 2] = np.where(counts[:, 0] > 0, np.nansum(weight, axis=(1, 2)) / np.maximum(counts[:, 0], 1), np.nan)
        return {"ba_weight": weight, "ba_counts": counts, "ba_params": {"loss": loss, "f_scale": f_scale, "cost": float(info["cost"]), "nfev": int(info["nfev"]),
                                                                          "status": int(info["status"]), "frame_stride": stride}}

    def calibration_outliers(self, threshold=0.5):
        """The detections the robust calibration disbelieved: a list of (camera id, image id, joint id) whose weight in the bundle
        adjustment ("ba_weight") is below `threshold` -- the detections to look at first, as outlier_cameras() lists them for the
        consensus.  Needs calibrate_calc() with a loss other than 'linear'; a rank-0 method."""
        from . import distributed as dd

        if dd.current()[0] != 0:
            raise RuntimeError("calibration_outliers is a rank-0 method: the camera network lives on rank 0")
        if getattr(self, "_ba_robust", None) is None:
            raise RuntimeError("calibration_outliers needs a robust calibration: run calibrate_calc(loss='soft_l1') first")
        if not (np.isfinite(threshold) and 0 < threshold <= 1):
            raise ValueError(f"threshold must lie in (0, 1] (it is {threshold:g})")
        with np.errstate(invalid="ignore"):
            return [(int(c), int(t), int(j)) for c, t, j in np.argwhere(self._ba_robust["ba_weight"] < threshold)]

    def get_points3d(self):
        """Pose for the 3-D video: array[image_id][joint_id] = (x, y, z) after Procrustes, median-centring + axis swap
        and the One-Euro temporal filter (reference :332-343), computed on the device."""
        return video_pose(np.copy(self.camNet.points3d), device=self.device)

    def save_corrections(self):
        """Write the manual corrections to the output folder (reference :345-347)."""
        self.db.dump()

    def _triangulate_sharded(self):
        """Multi-GPU form of the triangulation inside save(): the cameras are fixed by now (loaded from an earlier result, or
        adjusted by calibrate_calc on rank 0), so rank 0 broadcasts them -- one record of a flag + the seven 3 x 4 projection
        matrices -- every rank triangulates ITS frame range on its own GPU, and one gather brings points3d to rank 0
        (Procrustes is sequence-global and stays there).  Every rank calls this; returns [T, 38, 3] on rank 0, None on the
        others or when rank 0 holds no calibration.  Bit-identical to CameraNetwork.triangulate() on the gathered points."""
        import torch.distributed as dist

        from . import distributed as dd

        rank, world = dd.current()
        dev = dd.local_device() if self.device is None else torch.device(self.device)
        rec = torch.zeros(1 + 7 * 12, dtype=torch.float64)
        if rank == 0 and self.camNet is not None and self.camNet.has_calibration():
            rec[0] = 1.0
            rec[1:] = torch.from_numpy(np.stack([c.P for c in self.camNet.cam_list]).reshape(-1))
        wire = dd._wire_tensor(rec.to(dev), None)
        dist.broadcast(wire, src=0)
        rec = wire.cpu()
        if rec[0].item() == 0.0:
            return None
        t0, t1 = dd.shard_range(self.num_images, world, rank)
        scale = torch.tensor([float(v) for v in self.image_shape[::-1]], dtype=torch.float64, device=dev)
        # This rank's frames, in pixels.  A rank that holds a camera network (rank 0 after calibrate_calc; every rank after
        # reopening a result) reads them from IT, as CameraNetwork.triangulate() does single-GPU -- corrections written in place by
        # corrected_points2d_matrix() are then part of the triangulation; the other ranks use the shard their own inference left.
        px, bad = None, None
        if self.camNet is not None and self.camNet.points2d is not None and self.camNet.points2d.shape[1] == self.num_images:
            px = torch.from_numpy(np.ascontiguousarray(self.camNet.points2d[:, t0:t1])).to(dev)
        elif self._points2d_shard is not None:
            px = self._points2d_shard.to(dev) * scale
        elif self.points2d is not None:
            px = torch.from_numpy(np.ascontiguousarray(self.points2d[:, t0:t1])).to(dev) * scale
        if px is None or px.shape[1] != t1 - t0:
            # e.g. a reopened result whose length is not this run's num_images: NOT silently zeros (round-3 advisor finding) --
            # the collective below still runs well-formed, then every rank raises
            bad = ValueError(f"rank {rank}: {0 if px is None else px.shape[1]} frames of 2-D points for the frame range [{t0}, {t1}) of {self.num_images}")
            px = torch.zeros((7, t1 - t0, config["num_joints"], 2), dtype=torch.float64, device=dev)
        px = px.contiguous()
        # Manual corrections live in rank 0's camera network only (written in place by corrected_points2d_matrix()); the other
        # ranks triangulate from their raw inference shard.  Rank 0 therefore broadcasts the rows its correction store names, with
        # the values ITS table holds for them -- [cam, frame, J x 2 pixels] per row, two small broadcasts -- and every rank writes
        # the rows of its own frame range over its shard: the sharded result is then CameraNetwork.triangulate()'s, corrections
        # included, whichever rank owns the frame (round-4 advisor finding).
        J = config["num_joints"]
        rows = np.zeros((0, 2 + 2 * J))
        if rank == 0 and self.camNet is not None and self.camNet.points2d is not None and self.camNet.points2d.shape[1] == self.num_images:
            try:   # (a malformed correction entry must not leave the peers alone in the broadcasts below: it travels to agree())
                listed = [(int(c), int(i)) for c, per_image in self.db.manual_corrections().items() for i in per_image if c < config["num_cameras"] and i < self.num_images]
                if listed:
                    cams, frames = np.array([c for c, _ in listed]), np.array([i for _, i in listed])
                    rows = np.concatenate([cams[:, None], frames[:, None], self.camNet.points2d[cams, frames].reshape(len(listed), 2 * J)], axis=1).astype(np.float64)
            except Exception as e:  # noqa: BLE001
                bad, rows = bad or e, np.zeros((0, 2 + 2 * J))
        count = dd._wire_tensor(torch.tensor([rows.shape[0]], dtype=torch.int64).to(dev), None)
        dist.broadcast(count, src=0)
        if int(count.cpu()[0]):
            wire = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)) if rank == 0 else torch.zeros((int(count.cpu()[0]), 2 + 2 * J), dtype=torch.float64)
            wire = dd._wire_tensor(wire.to(dev), None)
            dist.broadcast(wire, src=0)
            table = wire.cpu()
            mine = (table[:, 1] >= t0) & (table[:, 1] < t1)
            if bool(mine.any()):   # one indexed assignment (rows of one (camera, frame) are unique: the store is a dict of dicts)
                table = table[mine]
                px[table[:, 0].long().to(px.device), (table[:, 1].long() - t0).to(px.device)] = table[:, 2:].reshape(-1, J, 2).to(px.device)
        X = ops.triangulate(rec[1:].reshape(7, 3, 4).numpy(), px) if t1 > t0 else torch.zeros((0, config["num_joints"], 3), dtype=torch.float64, device=dev)
        logger.debug(f"rank {rank} of {world}: triangulated frames [{t0}, {t1}) on {dev}")
        full = dd.gather_frames(X, 0, self.num_images)
        dd.agree(bad, "the sharded triangulation")
        return None if full is None else full.cpu().numpy()

    def save(self, joint_angles=False, rigid_legs=False, angle_spectrogram=False, behaviour_map=False, behaviour_perplexity=None,
             behaviour_segments=False, behaviour_sigma=None, behaviour_grid=None, gait=False, gait_on=None, gait_off=None, repair_pose=False,
             repair_window=None, repair_threshold=None, repair_floor=None, repair_max_gap=None, treadmill=False, ball_radius=None,
             check_sync=False, sync_cameras=False, sync_max_lag=None, sync_window=None, sync_tau=None, sync_switch=None, sync_min_count=None,
             heatmap_triangulation=False, heatmap_half=None, heatmap_levels=None, heatmap_floor=None,
             trajectory_triangulation=False, trajectory_lambda=None, trajectory_huber=None, trajectory_max_gap=None,
             robust_triangulation=False, robust_tau=None, robust_min_views=None):
        """Write df3d_result_*.pkl with the reference's schema and key order (reference :349-369).  `joint_angles=True` appends the
        keys "joint_angles" and "segment_lengths" (Core.joint_angles() of this save's triangulation; needs calibrated cameras).
        `rigid_legs=True` appends, after those, "points3d_rigid", "rigid_segment_lengths" and "rigid_fit_cost" (Core.rigid_legs()) and,
        together with joint_angles, "joint_angles_rigid" (Core.joint_angles(rigid=True)[0]).  `angle_spectrogram=True` appends,
        after all of those, "angle_spectrogram" [T, 6, 8, F] float32 (Core.angle_spectrogram() with its defaults),
        "spectrogram_freqs" [F], "spectrogram_fps" and, together with rigid_legs, "angle_spectrogram_rigid".  `behaviour_map=True`
        appends, after all of those, "behaviour_map" [T, 2] float64 (Core.behaviour_map() with its defaults and
        `behaviour_perplexity`), "behaviour_map_train_index", "behaviour_map_kl", "behaviour_map_perplexity" and, together with
        rigid_legs, "behaviour_map_rigid" and "behaviour_map_rigid_kl"; the spectrogram itself is stored only with angle_spectrogram.
        `behaviour_segments=True` (it needs behaviour_map) appends, after all of those, the segmentation of that same map
        (ops.segment_map with `behaviour_sigma` and `behaviour_grid`): "behaviour_density" [G, G], "behaviour_density_origin" (x0, y0, h),
        "behaviour_density_sigma", "behaviour_regions" [G, G] int32, "behaviour_region_peaks" [R, 2], "behaviour_labels" [T] int32,
        "behaviour_bouts" [B, 3], "behaviour_occupancy" and "behaviour_transitions" and, together with rigid_legs, the same nine with
        "_rigid" appended.  `gait=True` appends, after every other key, the gait analysis of this save's triangulation (Core.gait() with
        its defaults and the swing thresholds `gait_on` and `gait_off`): "gait_tip_position" and "gait_tip_velocity" [T, 6, 3],
        "gait_states" [T, 6] int8, "gait_steps" [S, 4], "gait_step_metrics" [S, 3], "gait_phase" [T, 6], "gait_coupling" [6, 6, 2],
        "gait_coupling_count" [6, 6], "gait_pattern" [T] int32, "gait_pattern_histogram" [64], "gait_state_counts" [6, 3],
        "gait_thresholds" (on, off, half_window) and "gait_fps" and, together with rigid_legs, the same thirteen with "_rigid" appended
        (of the fit this save computed, in the measured pose's recording frame).  `repair_pose=True` appends, after every other key,
        the repaired pose of this save's triangulation (Core.repair_pose() with `repair_window`, `repair_threshold`, `repair_floor`
        and `repair_max_gap`; the defaults are guesses nobody has measured on a recording): "points3d_repaired" [T, 38, 3],
        "repair_status" [T, 38] int8, "repair_counts" [38, 5], "repair_score" [T, 38] and "repair_params" (half_window, threshold,
        floor, max_gap, min_count); every other opt-in key of the same save is then computed from the repaired pose, which is repaired
        once.  "points3d" and "points3d_wo_procrustes" stay the triangulation's own.  `treadmill=True` appends, after the gait keys and
        before the repair keys, the treadmill ball and the fictive path of this save's triangulation (Core.treadmill() with its
        defaults and the known radius `ball_radius`, in mm; None fits the radius): "treadmill_ball_center" [3],
        "treadmill_ball_radius", "treadmill_ball_rms", "treadmill_ball_count", "treadmill_ball_status" (bit 0: refused),
        "treadmill_rotation" [T, 3], "treadmill_legs" [T] int32, "treadmill_residual" [T], "treadmill_fictive" [T, 3] (forward,
        sideways, yaw rate), "treadmill_path" [T, 3] (x, y, theta), "treadmill_skipped", "treadmill_params" (radius or NaN, on, off,
        half_window, min_legs, iterations) and "treadmill_fps".  There are no "_rigid" twins: the ball is one object.  Together with
        gait, the swing/stance states of the measured pose are computed once and shared.  After track_detections() the result holds,
        directly after "points2d_argmax", "track_choice" [7, T, 19] int8 (the slot every chain took in every frame), "track_cost"
        [7, 19] float64 (each chain's minimum) and "track_params" (tau, w_motion, w_value); without it no key is added.
        `robust_triangulation=True` appends, after every other key (after the repair keys), the consensus triangulation of the detections
        this save triangulates (Core.robust_triangulation() with `robust_tau`, pixels, one value or one per joint, and
        `robust_min_views`; the default tau is a guess nobody has measured on a recording): "points3d_robust" [T, 38, 3] in the layout
        of points3d_wo_procrustes, "robust_cameras" [T, 38] int32, "robust_status" [T, 38] int8, "robust_error" [7, T, 38],
        "robust_counts" [38, 4], "points2d_robust" [7, T, 38, 2] (the detections with every rejected view replaced by the projection of
        the robust point, divided by the image size like "points2d") and "robust_params" (the 38 values of tau, then min_views); every
        other opt-in key of the same save is then computed from the robust pose -- repaired afterwards with repair_pose -- which is
        computed once.  "points3d", "points3d_wo_procrustes" and "points2d" stay the plain triangulation's.
        `trajectory_triangulation=True` appends, after every other key (after the robust keys), the trajectory triangulation of the
        detections this save triangulates (Core.trajectory_triangulation() with `trajectory_lambda`, px^2 / mm^2, one value or one per
        joint, `trajectory_huber`, pixels, and `trajectory_max_gap`; the defaults are guesses nobody has measured on a recording):
        "points3d_trajectory" [T, 38, 3] in the layout of points3d_wo_procrustes, "trajectory_status" [T, 38] int8, "trajectory_weight"
        and "trajectory_error" [7, T, 38], "trajectory_iterations" [38], "trajectory_cost" [38, 2], "trajectory_counts" [38, 5] and
        "trajectory_params" (the 38 values of lambda, then huber, then max_gap).  The stages run in the order robust, trajectory,
        repair: together with robust_triangulation the fit starts from the robust points and sees only the views the consensus kept;
        every other opt-in key of the same save is computed from the trajectory pose (repaired afterwards with repair_pose), which is
        computed once.
        `heatmap_triangulation=True` appends, after every other key (after the trajectory keys), the heat-map triangulation of every
        frame (Core.heatmap_triangulation() with `heatmap_half`, mm, `heatmap_levels` and `heatmap_floor`; the defaults are guesses
        nobody has measured on a recording; the images must be present): "points3d_heatmap" [T, 38, 3] in the layout of
        points3d_wo_procrustes, "heatmap3d_status" [T, 38] int8, "heatmap3d_score" [T, 38], "heatmap3d_views" [T, 38] int32,
        "heatmap3d_shift" [T, 38], "heatmap3d_counts" [38, 4] and "heatmap3d_params" (half, levels, floor, grid).  The stages run in the
        order robust, trajectory, heat-map, repair: the search starts from the latest pose of the save, and every other opt-in key
        of the same save is computed from the heat-map pose (repaired afterwards with repair_pose), which is computed once.
        `check_sync=True` appends, after every other key (after the heat-map keys), the frame lags of the cameras (Core.camera_sync()
        with `sync_max_lag`, `sync_window`, `sync_tau`, `sync_switch` and `sync_min_count`; the defaults are guesses nobody has measured
        on a recording): "sync_lag" [7, nW] int32 (camera c shows instant t in its frame t + lag[c, t // window]), "sync_status" [7] int8
        (0 unobservable, 1 in step throughout, 2 lagging somewhere), "sync_pairs" [npair, 2], "sync_pair_lag" [npair, nW],
        "sync_pair_margin" [npair, nW] (px^2), "sync_pair_inconsistency" [npair, nW], "sync_pair_cost" [npair, nW, 2 max_lag + 1]
        (float64 px^2: the mean cost of a sample, NaN without one), "sync_pair_count" and "sync_params" (max_lag, window, tau, switch,
        min_count), and logs one line per lagging camera.  `sync_cameras=True` (it implies check_sync) also undoes the lags before the
        triangulation: "points2d", the triangulation and every later stage of this save hold the shifted detections (zeros where a
        camera has no such frame), and the originals follow the sync keys as "points2d_unsynced".  The object's own detections stay as
        they were.  Not after auto_correct() or track_detections() and not with heatmap_triangulation: those read heat-maps by frame
        index."""
        from . import distributed as dd
        from . import heatmap3d

        # a collective: every rank takes part.  After auto_correct() the peers hold only their raw (uncorrected) shards, so rank 0
        # triangulates every frame itself -- every rank knows that it ran (the flag is set on all of them) and takes this branch
        # (with sync_cameras too: the detections it triangulates are the shifted ones, which only rank 0 computes)
        pts3d_sharded = self._triangulate_sharded() if dd.current()[1] > 1 and not getattr(self, "_corrected", False) and not sync_cameras else None
        error = None
        if behaviour_segments and not behaviour_map:
            raise ValueError("behaviour_segments segments the map behaviour_map computes: it needs behaviour_map=True")
        if (behaviour_sigma is not None or behaviour_grid is not None) and not behaviour_segments:
            raise ValueError("behaviour_sigma and behaviour_grid belong to behaviour_segments: they need behaviour_segments=True")
        if (gait_on is not None or gait_off is not None) and not gait:
            raise ValueError("gait_on and gait_off belong to gait: they need gait=True")
        gait = dict(zip(("on", "off", "half_window"), ops.gait_thresholds(gait_on, gait_off))) if gait else None   # refused before any work
        if not repair_pose and any(v is not None for v in (repair_window, repair_threshold, repair_floor, repair_max_gap)):
            raise ValueError("repair_window, repair_threshold, repair_floor and repair_max_gap belong to repair_pose: they need repair_pose=True")
        repair = (dict(zip(("half_window", "threshold", "floor", "max_gap", "min_count"),
                           ops.repair_params(repair_window, repair_threshold, repair_floor, repair_max_gap))) if repair_pose else None)
        if ball_radius is not None and not treadmill:
            raise ValueError("ball_radius belongs to treadmill: it needs treadmill=True")
        treadmill = {"radius": ops.treadmill_params(ball_radius)[0]} if treadmill else None   # refused before any work
        if not robust_triangulation and (robust_tau is not None or robust_min_views is not None):
            raise ValueError("robust_tau and robust_min_views belong to robust_triangulation: they need robust_triangulation=True")
        robust = ops.consensus_params(robust_tau, robust_min_views) if robust_triangulation else None   # refused before any work
        if robust is not None and robust[0].shape not in ((1,), (config["num_joints"],)):
            raise ValueError(f"robust_tau must hold one value, or one per joint ({config['num_joints']})")
        if not trajectory_triangulation and any(v is not None for v in (trajectory_lambda, trajectory_huber, trajectory_max_gap)):
            raise ValueError("trajectory_lambda, trajectory_huber and trajectory_max_gap belong to trajectory_triangulation: "
                             "they need trajectory_triangulation=True")
        trajectory = (ops.trajectory_params(trajectory_lambda, trajectory_huber, trajectory_max_gap)
                      if trajectory_triangulation else None)   # refused before any work
        if trajectory is not None and trajectory[0].shape not in ((1,), (config["num_joints"],)):
            raise ValueError(f"trajectory_lambda must hold one value, or one per joint ({config['num_joints']})")
        if not heatmap_triangulation and any(v is not None for v in (heatmap_half, heatmap_levels, heatmap_floor)):
            raise ValueError("heatmap_half, heatmap_levels and heatmap_floor belong to heatmap_triangulation: they need heatmap_triangulation=True")
        heatmap = heatmap3d.heatmap3d_params(heatmap_half, heatmap_levels, heatmap_floor) if heatmap_triangulation else None   # refused before any work
        if not (check_sync or sync_cameras) and any(v is not None for v in (sync_max_lag, sync_window, sync_tau, sync_switch, sync_min_count)):
            raise ValueError("sync_max_lag, sync_window, sync_tau, sync_switch and sync_min_count belong to check_sync and sync_cameras: "
                             "they need one of them")
        if sync_cameras and (heatmap_triangulation or getattr(self, "_corrected", False)):
            raise ValueError("sync_cameras shifts the detections' frames: it cannot follow auto_correct() or track_detections() or be combined "
                             "with heatmap_triangulation, which read heat-maps by frame index")
        sync = ((sync_mod.sync_params(sync_max_lag, sync_window, sync_tau, sync_switch, sync_min_count), bool(sync_cameras))
                if check_sync or sync_cameras else None)   # refused before any work
        segments = (behaviour_sigma, behaviour_grid) if behaviour_segments else None
        if segments is not None:   # refused before any work
            if behaviour_grid is not None:
                ops._need_grid(behaviour_grid)
            if behaviour_sigma is not None and not (np.isfinite(behaviour_sigma) and behaviour_sigma > 0):
                raise ValueError(f"behaviour_sigma must be finite and > 0 (it is {behaviour_sigma:g})")
        if self.is_primary:
            try:
                self._write_result(pts3d_sharded, joint_angles, rigid_legs, angle_spectrogram, behaviour_map, behaviour_perplexity, segments, gait,
                                   repair, treadmill, robust, trajectory, heatmap, sync)
            except Exception as e:  # noqa: BLE001  (ENOSPC, a failing Procrustes, ...: re-raised by agree, on every rank)
                error = e
        dd.agree(error, "save")   # rank 0 failing here must not leave its peers in the NEXT step's collectives alone

    def _write_result(self, pts3d_sharded=None, joint_angles=False, rigid_legs=False, angle_spectrogram=False, behaviour_map=False,
                      behaviour_perplexity=None, segments=None, gait=None, repair=None, treadmill=None, robust=None, trajectory=None,
                      heatmap=None, sync=None):
        if behaviour_map and getattr(self, "num_images", None) is not None:   # too short for the perplexity: refused before any work
            ops.behaviour_map_points(self.num_images, behaviour_perplexity)
        if sync is None:
            return self._write_result_of(np.copy(self.points2d), {}, pts3d_sharded, joint_angles, rigid_legs, angle_spectrogram, behaviour_map,
                                         behaviour_perplexity, segments, gait, repair, treadmill, robust, trajectory, heatmap)
        r = self._sync_on("sync_cameras" if sync[1] else "check_sync", sync[0])
        sync_keys = self._sync_keys(r)
        if not sync[1]:
            return self._write_result_of(np.copy(self.points2d), sync_keys, pts3d_sharded, joint_angles, rigid_legs, angle_spectrogram,
                                         behaviour_map, behaviour_perplexity, segments, gait, repair, treadmill, robust, trajectory, heatmap)
        # the same gather on the normalised detections (exact: no arithmetic) is the result's "points2d"; the camera network holds the
        # shifted pixels while this save runs, so that every stage reads them, and gets its own back whatever happens
        shifted = sync_mod.apply_sync(torch.from_numpy(np.ascontiguousarray(self.points2d, dtype=np.float64)).to(r.points2d_px.device), r.lag,
                                 r.params[1]).cpu().numpy()
        sync_keys["points2d_unsynced"] = np.copy(self.points2d)
        own = np.copy(self.camNet.points2d)
        np.copyto(self.camNet.points2d, r.points2d_px.cpu().numpy())
        r = None
        try:
            return self._write_result_of(shifted, sync_keys, None, joint_angles, rigid_legs, angle_spectrogram, behaviour_map,
                                         behaviour_perplexity, segments, gait, repair, treadmill, robust, trajectory, heatmap)
        finally:
            np.copyto(self.camNet.points2d, own)
            self.camNet.triangulate()   # as every other save leaves it: the triangulation of the object's own detections

    def _write_result_of(self, points2d, sync_keys, pts3d_sharded, joint_angles, rigid_legs, angle_spectrogram, behaviour_map, behaviour_perplexity,
                         segments, gait, repair, treadmill, robust, trajectory, heatmap):
        """_write_result on `points2d` (normalised, the result's key; the camera network holds the same in pixels); `sync_keys` follow
        every other key."""
        result = {"points2d": points2d}
        if self.camNet is not None and self.camNet.has_calibration():
            if pts3d_sharded is not None:
                self.camNet.points3d = pts3d_sharded
            else:
                self.camNet.triangulate()
            pts3d = self.camNet.points3d
            result["points3d_wo_procrustes"] = pts3d
            result["points3d"] = procrustes_separate(pts3d, device=self.device)
            result = {**self.camNet.summarize(), **result}
        else:
            logger.debug("Triangulation skipped.")
        result["camera_ordering"] = self.camera_ordering
        result["heatmap_confidence"] = self.conf
        if getattr(self, "_corrected", False) and self.points2d_argmax is not None:
            result["points2d_argmax"] = np.copy(self.points2d_argmax)
            if getattr(self, "_track", None) is not None:   # track_detections() ran last: what it chose, directly after the arg-max detections
                result["track_choice"], result["track_cost"] = np.copy(self._track["choice"]), np.copy(self._track["cost"])
                result["track_params"] = np.copy(self._track["params"])
        if getattr(self, "_subpixel", False):   # only when this run refined its detections: without it the schema is the reference's
            result["subpixel"] = True
        # opt-in, like the two keys above: else the reference's schema
        if (joint_angles or rigid_legs or angle_spectrogram or behaviour_map or gait or repair or treadmill or robust is not None
                or trajectory is not None or heatmap is not None):
            result.update(self._kinematic_keys(joint_angles, rigid_legs, angle_spectrogram, behaviour_map, behaviour_perplexity, segments, gait,
                                               repair, treadmill, robust, trajectory, heatmap))
        if getattr(self, "_ba_robust", None) is not None:   # only after a robust calibration: else the schema is what it was
            result.update(self._ba_robust)
        result.update(sync_keys)
        with open(self.save_path, "wb") as f:
            pickle.dump(result, f)
        print(f"Saved results at: {self.save_path}")

    _KINEMATIC_KEYS = ("joint_angles", "segment_lengths", "points3d_rigid", "rigid_segment_lengths", "rigid_fit_cost", "joint_angles_rigid",
                       "angle_spectrogram", "spectrogram_freqs", "spectrogram_fps", "angle_spectrogram_rigid", "behaviour_map",
                       "behaviour_map_train_index", "behaviour_map_kl", "behaviour_map_perplexity", "behaviour_map_rigid", "behaviour_map_rigid_kl")
    _SEGMENT_KEYS = ("behaviour_density", "behaviour_density_origin", "behaviour_density_sigma", "behaviour_regions", "behaviour_region_peaks",
                     "behaviour_labels", "behaviour_bouts", "behaviour_occupancy", "behaviour_transitions")
    _KINEMATIC_KEYS += _SEGMENT_KEYS + tuple(k + "_rigid" for k in _SEGMENT_KEYS)

    _REPAIR_KEYS = ("points3d_repaired", "repair_status", "repair_counts", "repair_score", "repair_params")
    _ROBUST_KEYS = ("points3d_robust", "robust_cameras", "robust_status", "robust_error", "robust_counts", "points2d_robust", "robust_params")
    _TRAJECTORY_KEYS = ("points3d_trajectory", "trajectory_status", "trajectory_weight", "trajectory_error", "trajectory_iterations",
                        "trajectory_cost", "trajectory_counts", "trajectory_params")
    _HEATMAP3D_KEYS = ("points3d_heatmap", "heatmap3d_status", "heatmap3d_score", "heatmap3d_views", "heatmap3d_shift", "heatmap3d_counts",
                       "heatmap3d_params")

    def _kinematic_keys(self, joint_angles, rigid_legs, angle_spectrogram, behaviour_map, perplexity, segments=None, gait=None, repair=None,
                        treadmill=None, robust=None, trajectory=None, heatmap=None):
        """The keys save()'s flags append, in the result's order, all read from one PoseChain of this save's triangulation.
        `segments`: None, or (sigma, grid) of the segmentation of every map.  `gait`: None, or the thresholds of the gait analysis.
        `repair`: None, or the parameters of the pose repair; the one chain is then that of the repaired pose, repaired once.
        `treadmill`: None, or the parameters of the treadmill analysis; with `gait` it takes the measured pose's states from that.
        `robust`: None, or (tau, min_views) of the consensus triangulation; the one chain is then that of the robust pose (repaired
        afterwards when `repair` is set), computed once.  `trajectory`: None, or ops.trajectory_params' values of the trajectory
        triangulation, which runs after the consensus and before the repair; the one chain is then that of the trajectory pose.
        `heatmap`: None, or heatmap3d_params' values of the heat-map triangulation, which runs after the trajectory and before the
        repair from the latest pose; the one chain is then that of the heat-map pose."""
        what = ("joint_angles" if joint_angles else "rigid_legs" if rigid_legs else "angle_spectrogram" if angle_spectrogram
                else "behaviour_map" if behaviour_map else "gait" if gait is not None else "treadmill" if treadmill is not None
                else "repair_pose" if repair is not None else "robust_triangulation" if robust is not None else "trajectory_triangulation" if trajectory is not None
                else "heatmap_triangulation")
        spectra = angle_spectrogram or behaviour_map
        fps, bank = self._wavelet_bank(what, None, {}) if spectra else (None, {})   # save()'s fps and frequencies are the method's defaults
        if (gait is not None or treadmill is not None) and fps is None:
            fps = self._gait_fps(None)   # the same rule
        keys, host = {}, lambda t: t.cpu().numpy()
        robust_keys, trajectory_keys, pose, kept = {}, {}, None, None
        if robust is not None:
            r, px = self._robust_on(what, *robust, X=self.camNet.points3d)   # _write_result has just triangulated these detections
            kept = (r, px) if trajectory is not None else None   # the fit then sees the views the consensus kept, and starts from its points
            px = None
            scale = torch.tensor([float(v) for v in self.image_shape[::-1]], dtype=torch.float64, device=r.fixed_px.device)
            robust_keys = dict(zip(self._ROBUST_KEYS, (host(r.points3d), host(r.cameras), host(r.status), host(r.error), host(r.counts),
                                                       host(r.fixed_px / scale), np.append(r.params[0], float(r.params[1])))))
            pose, r = r.points3d, None
        if trajectory is not None:
            r = self._trajectory_on(what, trajectory, X=self.camNet.points3d, robust=kept)
            trajectory_keys = dict(zip(self._TRAJECTORY_KEYS, (host(r.points3d), host(r.status), host(r.weight), host(r.error), host(r.iterations),
                                                               host(r.cost), host(r.counts),
                                                               np.append(r.params[0], [float(r.params[1]), float(r.params[2])]))))
            pose, r, kept = r.points3d, None, None
        heatmap_keys = {}
        if heatmap is not None:
            r = self._heatmap3d_on(what, heatmap, X=self.camNet.points3d if pose is None else pose)
            heatmap_keys = dict(zip(self._HEATMAP3D_KEYS, (host(r.points3d), host(r.status), host(r.score), host(r.views), host(r.shift),
                                                           host(r.counts), np.array(r.params, dtype=np.float64))))
            pose, r = r.points3d, None
        chains = [self._measured_pose(what, fps, repair, pose)]
        pose = None
        repair_keys = {}
        if repair is not None:
            r = chains[0].repair
            repair_keys = dict(zip(self._REPAIR_KEYS, (host(r.points), host(r.status), host(r.counts), host(r.score),
                                                       np.array(r.params, dtype=np.float64))))
            r = None   # the chain alone holds the repaired pose on the device, and is dropped below
        if joint_angles:
            keys["joint_angles"], keys["segment_lengths"] = map(host, chains[0].angles)
        if rigid_legs:
            chains.append(chains[0].rigid())
            keys["points3d_rigid"], keys["rigid_fit_cost"] = host(chains[0].fit.points), host(chains[0].fit.cost)
            keys["rigid_segment_lengths"] = np.array(chains[0].fit.lengths)
            if joint_angles:
                keys["joint_angles_rigid"] = host(chains[1].angles[0])
        gait_keys, states = {}, None
        if gait is not None:   # the rigid chain is the fit computed above: it never runs twice
            for tag, chain in zip(("", "_rigid"), chains):
                g = chain.gait(**gait)
                if not tag and treadmill is not None:
                    states = g.states   # save()'s gait and treadmill share thresholds and window: the states are the same
                gait_keys.update({k + tag: v for k, v in zip(self._GAIT_KEYS, self._gait_values(g))})
                g = None
        if treadmill is not None:   # of the measured (or repaired) pose alone: the ball is one object
            shared = None if states is None else (gait["on"], gait["off"])
            gait_keys.update(zip(self._TREADMILL_KEYS, self._treadmill_values(chains[0].treadmill(states, **treadmill), shared)))
            states = None
        # The spectra read the [T, 48] series alone, and those wait on the host too (384 bytes per frame).  Everything the chains hold
        # is dropped with them, so that a map runs beside its own spectrogram and nothing else, as it did when every key started anew.
        dev = chains[0].points3d.device
        series = [c.series.unflatten(1, (6, 8)).cpu() for c in chains] if spectra else []
        del chains
        for tag in ("", "_rigid")[:len(series)]:
            S = ops.wavelet_spectrogram(series.pop(0).to(dev), fps, dtype=torch.float64 if behaviour_map else torch.float32, **bank)
            if angle_spectrogram:   # the float64 amplitude rounded once: by this cast where the map needs float64, else by the kernel
                keys["angle_spectrogram" + tag] = host(S.to(torch.float32))
            if behaviour_map:
                m = ops.behaviour_map(S, perplexity)
                keys["behaviour_map" + tag], keys[f"behaviour_map{tag}_kl"] = host(m.embedding), m.kl
                if not tag:
                    keys["behaviour_map_train_index"], keys["behaviour_map_perplexity"] = host(m.train_index), m.perplexity
                if segments is not None:   # of the map just computed: the t-SNE never runs twice
                    s = ops.segment_map(m.embedding, segments[1], segments[0])
                    values = (host(s.density), np.array(s.origin), s.sigma, host(s.regions), host(s.region_peaks), host(s.labels), host(s.bouts),
                              host(s.occupancy), host(s.transitions))
                    keys.update({k + tag: v for k, v in zip(self._SEGMENT_KEYS, values)})
                    s = None
            S = m = None   # released before the other variant's is computed: one float64 spectrogram at a time
        if angle_spectrogram:
            keys["spectrogram_freqs"], keys["spectrogram_fps"] = bank["freqs"], fps
        return {**{k: keys[k] for k in self._KINEMATIC_KEYS if k in keys}, **gait_keys, **repair_keys, **robust_keys, **trajectory_keys,
                **heatmap_keys}

    # -- helpers --------------------------------------------------------------------------------------
    def _correction_for(self, corrections, cam_id, img_id):
        return corrections.get(cam_id, {}).get(img_id)

    def corrected_points2d(self, cam_id, img_id):
        """Joints of one image in pixels: the manual correction when one is stored, else the estimate
        (reference df3d/core.py:374-385)."""
        estimate = self.camNet.cam_list[cam_id][img_id].copy()
        fix = self._correction_for(self.db.manual_corrections(), cam_id, img_id)
        if fix is not None:
            estimate[:] = fix
        return estimate

    def corrected_points2d_matrix(self):
        """results[cam_id][img_id][joint_id] = (row, col), stored corrections written over the camera network's
        estimates -- in place, like the reference (df3d/core.py:387-401)."""
        corrections = self.db.manual_corrections()
        everything = self.camNet.points2d
        self.camNet.drop_smoothed()
        for cam_id, per_image in corrections.items():
            for img_id, fix in per_image.items():
                if cam_id < config["num_cameras"] and img_id < self.num_images:
                    everything[cam_id, img_id, :] = fix
        return everything

    def setup_camera_ordering(self, camera_ordering) -> np.ndarray:
        order = find_default_camera_ordering(self.input_folder) if camera_ordering is None else camera_ordering
        return np.array(order)

    def plot_2d(self, cam_id, img_id, with_corrections=False, smooth=False, joints=[]):
        """Image `img_id` of camera `cam_id` with its 2-D pose drawn on it, as an ndarray (reference df3d/core.py:298-319).
        Host-side drawing.  `smooth=True` draws the temporally smoothed estimate (smooth_points2d) instead of the estimate;
        with `with_corrections=True` a stored manual correction of the image wins over either.  `joints` restricts the drawing to
        the listed joint ids."""
        from .config import skeleton_bones

        pts = np.array((self.smooth_points2d(cam_id) if smooth else self.camNet.cam_list[cam_id])[img_id], dtype=np.float64)
        fix = self._correction_for(self.db.manual_corrections(), cam_id, img_id) if with_corrections else None
        if fix is not None:
            pts[:] = fix
        if len(joints):
            keep = np.zeros(len(pts), dtype=bool)
            keep[list(joints)] = True
            pts = np.where(keep[:, None], pts, 0.0)
        return self.camNet[cam_id].plot_2d(img_id, points2d=pts, bones=skeleton_bones())

    # -- heat-map overlays (the reference's README lists plot_heatmap / has_heatmap, its 1.0.1 has no body for them) ----
    @property
    def has_heatmap(self):
        """Whether plot_heatmap() can draw: true while the image files are present.  Heat-maps are recomputed from the images on demand
        (heatmaps()), never stored: a recording's heat-maps are 4.3 MB per image, and after delete_images() there is nothing to compute
        them from."""
        try:
            for cam in range(config["num_cameras"]):
                image_path_for(self.input_folder, cam, 0)
        except FileNotFoundError:
            return False
        return True

    def _heatmap_views(self, img_id):
        from . import distributed as dd
        from . import jpeg
        from .inference import PREPROCESS, get_engine

        if dd.current()[0] != 0:
            raise RuntimeError("the heat-map queries are rank-0 methods, like the reprojection-error queries")
        img_id = int(img_id)
        if not 0 <= img_id < self.num_images:
            raise IndexError(f"image ids must lie in [0, {self.num_images})")
        if self._heatmap_cache is not None and self._heatmap_cache[0] == img_id:
            return self._heatmap_cache
        ncam = config["num_cameras"]
        blobs = []
        for cam in range(ncam):
            with open(image_path_for(self.input_folder, cam, img_id), "rb") as f:
                blobs.append(f.read())
        engine = get_engine(dtype=self.dtype, device=self.device)
        W, H = self.image_shape
        luma = jpeg.decode_luma(blobs, W, H, device=engine.device)
        flip = torch.tensor([1 if camera_is_flipped(cam, self.camera_ordering) else 0 for cam in range(ncam)], dtype=torch.uint8, device=engine.device)

        def forward(e):
            return e.forward_u8(luma, flip, PREPROCESS["mean"], PREPROCESS["std"], resize=PREPROCESS["resize"])

        if engine.dtype != "f32" and not self._heatmap_proven:   # as inference_folder proves a reduced-precision engine on its first views
            engine.canary(get_engine(dtype="f32", device=self.device), forward, what=f"image {img_id} of {self.input_folder}")
            self._heatmap_proven = True
        self._heatmap_cache = (img_id, luma, forward(engine))
        return self._heatmap_cache

    def heatmaps(self, img_id):
        """[7, 19, 64, 128] float32 CUDA tensor: the network's heat-maps of image `img_id`, camera by camera, as the network saw the
        view (cameras after position 3 of the camera ordering mirrored).  Computed on demand on pose2d_estimation's own path -- the
        same file bytes, device JPEG decode, flip set, preprocessing and `dtype` engine (a reduced-precision engine first proves itself
        against the exact one, HourglassEngine.canary) -- so they are the heat-maps the run took its detections from.  The last image's
        result is kept (a one-entry cache): treat it as read-only.  A rank-0 method."""
        return self._heatmap_views(img_id)[2]

    def plot_heatmap(self, cam_id, img_id, joints=[], gain=1.0):
        """Image `img_id` of camera `cam_id` with its heat-maps drawn on it, [H, W, 3] uint8 ndarray (the reference README's
        `Core.plot_heatmap(cam_id, img_id, joints=[])`; the drawing rule is DESIGN.md section 13): every pixel is tinted with the
        colour of the joint whose heat-map is largest there, the stronger the larger the value, so a plane's peak lies where plot_2d
        draws the detection.  `joints` restricts the drawing to the listed ids of the 38-joint layout (plot_2d's); joints the camera
        does not fill are ignored, and the front camera, which fills none, gives the grey image.  `gain` multiplies the heat-maps before
        they are clamped to [0, 1]."""
        _, luma, hm = self._heatmap_views(img_id)
        pairs = heatmap_planes(cam_id, joints, self.camera_ordering)
        img = ops.render_heatmap(luma[cam_id], hm[cam_id], [p for p, _ in pairs], [plane_color(j) for _, j in pairs],
                                 camera_is_flipped(cam_id, self.camera_ordering), gain=gain)
        return img.cpu().numpy()

    def get_image(self, cam_id, img_id):
        return self.camNet.cam_list[cam_id].get_image(img_id)

    def get_fps(self):
        """Frame rate of the camera videos (ffprobe on each of them; a warning when they differ, the first one wins),
        None without videos, without ffprobe or when an answer cannot be parsed (reference df3d/core.py:403-428)."""
        rates = []
        for video in camera_videos(self.input_folder):
            cmd, answer = probe_frame_rate(video)
            if answer is None:
                logger.warning(f"Command failed: {' '.join(cmd)}")
                return None
            rate = parse_frame_rate(answer)
            if rate is None:
                logger.warning(f'Could not parse framerate "{answer}" returned by ffprobe, so setting fps to None.')
                return None
            rates.append(rate)
        if len(set(rates)) > 1:
            logger.warning(f"The camera videos have different frame rates {rates}; using {rates[0]}.")
        return rates[0] if rates else None

    def expand_videos(self):
        """camera_x.mp4 -> camera_x_img_y.jpg through ffmpeg for cameras whose frames are not there yet."""
        for video in camera_videos(self.input_folder):
            cam_id = parse_vid_name(os.path.basename(video))
            first_frames = (os.path.join(self.input_folder, f"camera_{cam_id}_img_{n}.jpg") for n in ("0", "000000"))
            if not any(os.path.exists(f) for f in first_frames):
                extract_frames(video, self.input_folder, cam_id)

    def delete_images(self):
        """Remove the expanded frames of every camera that still has its .mp4.  Multi-GPU: every rank must have finished
        reading its shard first (the gather is not a barrier for the senders), and only rank 0 deletes."""
        from . import distributed as dd

        if dd.current()[1] > 1:
            torch.distributed.barrier()
        if not self.is_primary:
            return
        for video in camera_videos(self.input_folder, any_id=False):
            cam_id = parse_vid_name(os.path.basename(video))
            for frame in glob.glob(os.path.join(self.input_folder, f"camera_{cam_id}_img_*.jpg")):
                try:
                    os.remove(frame)
                except FileNotFoundError:
                    pass
