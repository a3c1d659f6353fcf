"""`PoseChain`: the kinematic chain of one triangulated pose (DESIGN.md sections 14-19) -- body frame, joint angles, leg fit,
unwrapping, wavelet spectrogram, behaviour map, its segmentation, the gait analysis and the treadmill ball (section 21), and the
repair of the pose itself (section 20) -- with every stage that the default arguments reach computed once.

A chain lives for one call of `Core`: each stage once per save, nothing kept between calls, because `camNet.points3d` changes under
corrections and re-triangulation.  It keeps the small products (frame, fit, angles, the 48 series: a few KB per frame).  The
float64 spectrogram, 10 KB per frame, is never kept: whoever asks for it holds it, and two never live side by side.
"""
from functools import cached_property

import torch

from . import config, logger, ops


def _recording(body_frame):
    return isinstance(body_frame, str) and body_frame == "recording"


def _unwrapped(series):
    names = config.LEG_ANGLE_NAMES
    cols = [8 * leg + names.index(a) for leg in range(6) for a in config.SPECTROGRAM_UNWRAPPED_ANGLES]
    series, left = ops.unwrap_phase(series, cols)
    if left:
        logger.warning("angle_spectrogram: not unwrapped, because they hold a non-finite sample: "
                       + ", ".join(f"{config.LEG_NAMES[c // 8]} {names[c % 8]}" for c in left))
    return series


class PoseChain:
    """The chain of `points3d` [T, 38, 3] float64 cuda (the layout of points3d_wo_procrustes) sampled at `fps` (needed by the
    spectrogram and the gait analysis alone).  The attributes are the products of the default arguments, computed on first use; a
    method called with other arguments computes what it is asked for directly from `ops` and keeps nothing.  `measured`: the chain
    whose recording frame this one shares (see rigid()).  `repair`: the ops.PoseRepairResult this pose came from (see repaired())."""

    def __init__(self, points3d, fps=None, measured=None, repair=None):
        self.points3d, self.fps, self.measured, self.repair = points3d, fps, measured, repair

    @cached_property
    def frame(self):
        """[1, 3, 3]: the recording's body frame.  A pose without frames has no medians to take: there it is the word "recording"
        itself, which ops.joint_angles answers with empty arrays."""
        if self.measured is not None:
            return self.measured.frame
        return ops.recording_frame(self.points3d) if self.points3d.shape[0] else "recording"

    @cached_property
    def fit(self):
        """ops.fit_legs' LegFitResult with its defaults."""
        return ops.fit_legs(self.points3d)

    def rigid(self):
        """A chain of the fitted pose, in the recording frame of THIS, the measured, pose: both sets of angles share one frame.  The
        fit is this chain's and computed once; the new chain's products are its own, so hold it."""
        return PoseChain(self.fit.points, self.fps, measured=self)

    def repaired(self, **params):
        """A chain of the repaired pose (ops.repair_pose; `params`: half_window, threshold, floor, max_gap, min_count), which keeps the
        PoseRepairResult as `repair`.  Unlike rigid(), the new chain has its own recording frame -- the frame should profit from the
        repair -- and its rigid() fits the repaired pose.  The repair is computed here, once: hold the chain."""
        r = ops.repair_pose(self.points3d, **params)
        return PoseChain(r.points, self.fps, repair=r)

    @cached_property
    def angles(self):
        """(angles [T, 6, 8], lengths [T, 6, 4]) in the recording frame."""
        return ops.joint_angles(self.points3d, self.frame)

    def joint_angles(self, body_frame="recording"):
        return self.angles if _recording(body_frame) else ops.joint_angles(self.points3d, body_frame)

    @cached_property
    def series(self):
        """[T, 48]: the recording-frame angles as time series, those of config.SPECTROGRAM_UNWRAPPED_ANGLES unwrapped
        (ops.unwrap_phase; the series left wrapped are named in one logged warning)."""
        return _unwrapped(self.angles[0].reshape(self.points3d.shape[0], 48))

    def spectrogram(self, body_frame="recording", unwrap=True, dtype=torch.float64, **bank):
        """[T, 6, 8, F] of `dtype`: ops.wavelet_spectrogram(series, fps, **bank) of the 48 series.  Not kept."""
        if self.fps is None:
            raise ValueError("this chain was built without the recording's fps, which the spectrogram needs")
        T = self.points3d.shape[0]   # (named: an empty pose leaves reshape(-1, ...) ambiguous)
        if unwrap and _recording(body_frame):
            series = self.series
        else:
            series = self.joint_angles(body_frame)[0].reshape(T, 48)
            series = _unwrapped(series) if unwrap else series
        return ops.wavelet_spectrogram(series.reshape(T, 6, 8), self.fps, dtype=dtype, **bank)

    def behaviour_map(self, perplexity=None, n_iter=None, max_points=None, seed=0, **spectrogram_kwargs):
        """ops.behaviour_map of the float64 spectrogram(**spectrogram_kwargs)."""
        return ops.behaviour_map(self.spectrogram(**spectrogram_kwargs), perplexity, n_iter, max_points, seed)

    def behaviour_segments(self, grid=None, sigma=None, min_peak=None, **behaviour_map_kwargs):
        """(the BehaviourMapResult, ops.segment_map of its embedding): one map, computed once, and its segmentation."""
        m = self.behaviour_map(**behaviour_map_kwargs)
        return m, ops.segment_map(m.embedding, grid, sigma, min_peak)

    def gait(self, **thresholds):
        """ops.gait (a GaitResult) of this pose at this chain's fps in the recording frame; `thresholds`: on, off, half_window.
        Not kept."""
        if self.fps is None:
            raise ValueError("this chain was built without the recording's fps, which the tip velocity needs")
        return ops.gait(self.points3d, self.fps, self.frame, **thresholds)

    def treadmill(self, states=None, **params):
        """ops.treadmill (a TreadmillResult) of this pose at this chain's fps in the recording frame; `states`: the states of a gait
        analysis of this pose that its caller already holds; `params`: radius, on, off, half_window, min_legs, iterations.  Not kept."""
        if self.fps is None:
            raise ValueError("this chain was built without the recording's fps, which the tip velocity needs")
        return ops.treadmill(self.points3d, self.fps, self.frame, states, **params)
