"""Heat-map triangulation: the 3-D point of every (frame, joint) is searched where the product of the views'
heat-maps, sampled at the point's projection, is largest.  Host wrappers over csrc/heatmap3d.hip in the manner of ops.py (whose public
surface is pinned and stays as it is): inputs and outputs are torch CUDA tensors, every computation is a libdf3d_hip.so kernel, and
there is no CPU fallback.  The model is stated in float64 numpy by tests/heatmap3d_oracle.py.
"""
import ctypes
import dataclasses

import numpy as np
import torch

from . import _native, config
from .ops import _call, _camera_matrices, _integer, _need, _number, _on_tensor_device, _stream


@dataclasses.dataclass
class HeatmapTriangulation:
    """What `triangulate_heatmaps` returns, device tensors but for params: points3d [n, J, 3] float64, score [n, J] float64 (the sum of
    the views' log heat-maps at the point; NaN for status 0), status [n, J] int8 (0 fewer than two views or no start point: the bits of
    X0, 1 searched, 2 no evidence within the cube: X0, 3 searched, and the best point of the first level lay on a face of the cube, which
    may be too small), views [n, J] int32 (bit v: view v has a plane for the joint), shift [n, J] float64 (|point - X0|, mm), choice
    [n, J, levels] int32 (the index of the point chosen at every level, -1 where none was), counts [J, 4] int64 (how often each status
    occurred per joint), params (half, levels, floor, grid) and path [n, J] int8 (0 not searched, 1 the search read its windows from
    LDS, 2 from the planes)."""
    points3d: torch.Tensor
    score: torch.Tensor
    status: torch.Tensor
    views: torch.Tensor
    shift: torch.Tensor
    choice: torch.Tensor
    counts: torch.Tensor
    params: tuple
    path: torch.Tensor = None


def heatmap3d_params(half=None, levels=None, floor=None):
    """(half, levels, floor) with config.HEATMAP3D_HALF (mm), config.HEATMAP3D_LEVELS and config.HEATMAP3D_FLOOR for what is None --
    guesses nobody has measured on a recording.  ValueError: a half that is no finite number > 0, a levels that is no integer in
    config.HEATMAP3D_LEVELS_RANGE, a floor that is no number with 0 < floor < 1."""
    h = _number(config.HEATMAP3D_HALF if half is None else half, "half", positive=True)
    n = _integer(config.HEATMAP3D_LEVELS if levels is None else levels, *config.HEATMAP3D_LEVELS_RANGE, "levels")
    f = _number(config.HEATMAP3D_FLOOR if floor is None else floor, "floor")
    if not 0.0 < f < 1.0:
        raise ValueError(f"floor must be a number with 0 < floor < 1 (it is {floor!r})")
    return h, n, f


def window_doubles():
    """The most float64 cells one (frame, joint) stages in LDS (df3d_heatmap3d_window_doubles): beyond it the search reads the planes."""
    return int(_native.load().df3d_heatmap3d_window_doubles())


def view_table(camera_ordering=None):
    """(cameras [6], flip [6] uint8, plane [6, 38] int32): the cameras that have heat-map planes under `camera_ordering` (default: the
    identity) in ascending camera id, whether the network sees each of them mirrored (config.camera_is_flipped), and the plane of every
    joint of the 38-joint layout in each of them (config.heatmap_planes), -1 where the camera does not fill the joint."""
    cameras, flip, plane = [], [], []
    for cam in range(config.config["num_cameras"]):
        pairs = config.heatmap_planes(cam, (), camera_ordering)
        if not pairs:
            continue
        row = np.full(config.config["num_joints"], -1, dtype=np.int32)
        for p, j in pairs:
            row[j] = p
        cameras.append(cam), flip.append(1 if config.camera_is_flipped(cam, camera_ordering) else 0), plane.append(row)
    return np.array(cameras, dtype=np.int64), np.array(flip, dtype=np.uint8), np.stack(plane)


def _inputs(P, heatmaps, flip, plane, image_shape):
    """(Ph, flip, plane, n, V, C, H, W, J, cell_rows, cell_cols) of heatmaps [n, V, C, H, W] and the tables of its V views."""
    _need(heatmaps, torch.float32, "heatmaps")
    if heatmaps.dim() != 5:
        raise ValueError("heatmaps must be [n, V, C, H, W]")
    n, V, C, H, W = (int(v) for v in heatmaps.shape)
    flip = np.ascontiguousarray(np.asarray(flip) != 0, dtype=np.uint8).reshape(-1)
    plane = np.ascontiguousarray(plane, dtype=np.int32)
    if not 1 <= V <= 8 or flip.shape != (V,) or plane.ndim != 2 or plane.shape[0] != V or not 1 <= plane.shape[1] <= 64:
        raise ValueError("heatmaps must hold 1 to 8 views, flip one entry per view, and plane [V, J] 1 to 64 joints")
    Ph = _camera_matrices(P, V)
    return Ph, flip, plane, n, V, C, H, W, plane.shape[1], float(image_shape[1]) / H, float(image_shape[0]) / W


_DP, _BP, _IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)


@_on_tensor_device
def heatmap_scores(P, heatmaps, flip, plane, points, image_shape, floor=None):
    """score [n, J, M] float64 cuda of the 3-D points `points` [n, J, M, 3] float64 cuda (df3d_heatmap3d_scores):
    the sum over the joint's views of the Catmull-Rom sample of the view's log heat-map at the point's projection.  Arguments as
    triangulate_heatmaps.  For tests: the sampler alone."""
    f = heatmap3d_params(floor=floor)[2]
    Ph, flip, plane, n, V, C, H, W, J, cell_rows, cell_cols = _inputs(P, heatmaps, flip, plane, image_shape)
    _need(points, torch.float64, "points")
    if points.dim() != 4 or tuple(points.shape[:2]) != (n, J) or points.shape[3] != 3 or points.device != heatmaps.device:
        raise ValueError("points must be [n, J, M, 3] on the heat-maps' device")
    M = int(points.shape[2])
    out = torch.empty((n, J, M), dtype=torch.float64, device=heatmaps.device)
    _call("df3d_heatmap3d_scores", heatmaps.data_ptr(), n, V, C, H, W, Ph.ctypes.data_as(_DP), flip.ctypes.data_as(_BP), plane.ctypes.data_as(_IP),
          J, points.data_ptr(), M, cell_rows, cell_cols, float(np.log(f)), out.data_ptr(), _stream(heatmaps))
    return out


@_on_tensor_device
def triangulate_heatmaps(P, heatmaps, flip, plane, X0, image_shape, half=None, levels=None, floor=None, budget=None):
    """The 3-D point of every (frame, joint) where the product of its views' heat-maps is largest (df3d_triangulate_heatmaps, DESIGN.md
    section 25), a HeatmapTriangulation.  heatmaps [n, V, C, H, W] float32 cuda, as the network saw the views; P [V, 3, 4] float64 (numpy
    or tensor, pixels); flip [V]: whether the network saw the view mirrored; plane [V, J] int32: the plane of joint j in view v or -1
    (view_table gives both for the fly); X0 [n, J, 3] float64 cuda: the start points, the plain triangulation; image_shape [W, H] of the
    camera images.  `levels` levels of 8 x 8 x 8 points, the first in the cube of half width `half` (mm) around X0, each next one around
    the best point with the step as half width; a cell at or below `floor` counts as the floor.  A joint with fewer than two views, or
    whose X0 is zero or not finite, keeps X0.  With two views two blobs in one view cannot be told apart: the stronger wins.  `budget`
    (tests): the most cells a workgroup stages in LDS, at most window_doubles(), the default; both routes give the same bits.
    Defaults and refusals: heatmap3d_params."""
    h, lv, f = heatmap3d_params(half, levels, floor)   # refused before any device work
    Ph, flip, plane, n, V, C, H, W, J, cell_rows, cell_cols = _inputs(P, heatmaps, flip, plane, image_shape)
    _need(X0, torch.float64, "X0")
    dev = heatmaps.device
    if tuple(X0.shape) != (n, J, 3) or X0.device != dev:
        raise ValueError("X0 must be [n, J, 3] on the heat-maps' device")
    budget = window_doubles() if budget is None else _integer(budget, 0, window_doubles(), "budget")
    out = HeatmapTriangulation(torch.empty((n, J, 3), dtype=torch.float64, device=dev), torch.empty((n, J), dtype=torch.float64, device=dev),
                               torch.empty((n, J), dtype=torch.int8, device=dev), torch.empty((n, J), dtype=torch.int32, device=dev),
                               torch.empty((n, J), dtype=torch.float64, device=dev), torch.empty((n, J, lv), dtype=torch.int32, device=dev),
                               torch.zeros((J, 4), dtype=torch.int64, device=dev), (h, lv, f, config.HEATMAP3D_GRID),
                               torch.empty((n, J), dtype=torch.int8, device=dev))
    _call("df3d_triangulate_heatmaps", heatmaps.data_ptr(), n, V, C, H, W, Ph.ctypes.data_as(_DP), flip.ctypes.data_as(_BP),
          plane.ctypes.data_as(_IP), J, X0.data_ptr(), h, lv, cell_rows, cell_cols, float(np.log(f)), budget, out.points3d.data_ptr(),
          out.score.data_ptr(), out.status.data_ptr(), out.views.data_ptr(), out.shift.data_ptr(), out.choice.data_ptr(), out.counts.data_ptr(),
          out.path.data_ptr(), _stream(heatmaps))
    return out
