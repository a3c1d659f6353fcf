"""Thin host wrappers over the C ABI for the non-network kernels: arg-max and peaks, re-layout, triangulation, Procrustes and the
video pose, and what DESIGN.md sections 9-24 add -- pictorial structures, reprojection errors, 2-D smoothing, the heat-map
overlay, joint angles, the leg fit, wavelet spectrograms, behaviour maps, their segmentation, the gait analysis, the pose repair,
the treadmill ball, the tracking of the detections through time, the consensus triangulation over camera subsets and the trajectory
triangulation.

Inputs/outputs are torch CUDA tensors (device memory + stream plumbing only); every computation is a
libdf3d_hip.so kernel.  No CPU fallback: a missing library or GPU raises `_native.NativeLibraryError`.

Every rule that more than one family applies to its arguments is written once, in the block below the imports: the tensor checks
(`_need`, strict, and `_need_tensor`, which returns the contiguous tensor that the caller then uses), the camera matrices, the
inputs of the triangulations, the `body_frame` argument, the workspace query, the integer / number / per-joint parameters, and
`_call`, the call path that turns the library's DF3D_EINVAL into a ValueError.  A new family takes its checks from there and keeps
only its own refusal texts.
"""
import collections
import ctypes
import dataclasses

import numpy as np
import torch

from . import _native


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _on_tensor_device(fn):
    """Kernels are launched on the calling thread's CURRENT HIP device: make that the device of the first tensor
    argument, so a process that drives several GPUs (or one that never called torch.cuda.set_device) stays correct."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kw):
        for a in args:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                with torch.cuda.device(a.device):
                    return fn(*args, **kw)
        return fn(*args, **kw)

    return wrapper


def _need(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor")


def _need_tensor(t, dtype, tail, name):
    """`t`, contiguous: a `dtype` CUDA tensor of shape [T, *tail] and any strides.  The caller goes on with what this returns."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 1 + len(tail) and tuple(t.shape[1:]) == tuple(tail)):
        raise ValueError(f"{name} must be a {dtype} CUDA tensor of shape [{', '.join(['T', *(str(n) for n in tail)])}]")
    return t.contiguous()


def _camera_matrices(P, ncam):
    """P [ncam, 3, 4] (numpy or tensor) as a contiguous float64 host array."""
    Ph = np.ascontiguousarray(P.detach().cpu().numpy() if isinstance(P, torch.Tensor) else P, dtype=np.float64)
    if Ph.shape != (ncam, 3, 4):
        raise ValueError("P must be [ncam, 3, 4]")
    return Ph


def _need_points2d_px(points2d_px, bounded=False):
    """(ncam, T, J) of points2d_px [ncam, T, J, 2], contiguous float64 cuda; `bounded`: within the 8 cameras and 64 joints of the consensus and trajectory kernels."""
    _need(points2d_px, torch.float64, "points2d_px")
    if points2d_px.dim() != 4 or points2d_px.shape[3] != 2:
        raise ValueError("points2d_px must be [ncam, T, J, 2]")
    ncam, T, J, _ = points2d_px.shape
    if bounded and not (1 <= ncam <= 8 and 1 <= J <= 64):
        raise ValueError("points2d_px must hold 1 to 8 cameras and 1 to 64 joints")
    return ncam, T, J


def _need_X(X, points2d_px):
    """An explicit X [T, J, 3], contiguous float64, on the frames, joints and device of points2d_px [ncam, T, J, 2]."""
    _need(X, torch.float64, "X")
    if tuple(X.shape) != (*points2d_px.shape[1:3], 3) or X.device != points2d_px.device:
        raise ValueError("X must be [T, J, 3] on the device of points2d_px")


_BODY_FRAME_TEXT = ('body_frame must be "recording", "per_frame" or a [3, 3] / [T, 3, 3] array',
                    "an explicit body_frame must be [3, 3] or [T, 3, 3] with T = {T}")


def _body_frames(value, T, dev, per_frame_allowed=True, text=_BODY_FRAME_TEXT):
    """The `body_frame` argument of a family: None for "recording" and, where allowed, "per_frame" -- `_fill_body_frames` computes
    those once the caller knows that there are frames --, else the explicit [3, 3] or, where allowed, [T, 3, 3] array or tensor as
    contiguous float64 frames [1 or T, 3, 3] on `dev`.  `text`: the refusals of the string and of the shape."""
    if isinstance(value, str):
        if value != "recording" and not (per_frame_allowed and value == "per_frame"):
            raise ValueError(text[0])
        return None
    frames = value if isinstance(value, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64))
    if tuple(frames.shape) not in ((3, 3), (1, 3, 3)) + (((T, 3, 3),) if per_frame_allowed else ()):
        raise ValueError(text[1].format(T=T))
    return frames.to(device=dev, dtype=torch.float64).reshape(-1, 3, 3).contiguous()


def _fill_body_frames(frames, value, points3d):
    """`frames` of _body_frames, with None replaced by the frames that `value` names, of points3d [T >= 1, 38, 3]."""
    if frames is not None:
        return frames
    return recording_frame(points3d) if value == "recording" else body_frame(points3d)


def _workspace(entry_name, *dims, device, refusal=None, least=0):
    """(work, need): the `need` bytes that the library's `entry_name`(*dims) asks for, as a uint8 tensor of at least `least` bytes on
    `device` (None: no tensor, the size alone).  A size <= 0 is the entry's refusal of `dims`: ValueError with
    `refusal`.format(*dims), by default the library's own message."""
    lib = _native.load()
    need = getattr(lib, entry_name)(*dims)
    if need <= 0:
        raise ValueError(lib.df3d_last_error().decode() if refusal is None else refusal.format(*dims))
    return (None if device is None else torch.empty((max(need, least),), dtype=torch.uint8, device=device)), need


def _integer(v, lo, hi, name):
    """int(v) of a Python or numpy integer (no bool, no float) in [lo, hi]."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}] (it is {v!r})")
    return int(v)


def _number(v, name, positive=False):
    """float(v) of a Python or numpy real number (no bool, no string); `positive`: a finite one > 0."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or (positive and not (np.isfinite(v) and v > 0)):
        raise ValueError(f"{name} must be {'a finite number > 0' if positive else 'a number'} (it is {v!r})")
    return float(v)


def _per_joint(value, default, name, finite=False):
    """A float64 array of one value or of one per joint from `value` (a number or a sequence of numbers; None: `default`), every
    one >= 0 and not NaN -- `finite`: nor +inf.  `_broadcast_per_joint` fits it to the J of the data."""
    if value is None:
        a = np.array(default, dtype=np.float64)
    else:
        if isinstance(value, (bool, str)) or (isinstance(value, (list, tuple, np.ndarray)) and np.asarray(value).dtype.kind not in "fiu"):
            raise ValueError(f"{name} must be a number or one number per joint (it is {value!r})")
        try:
            a = np.array(value, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number or one number per joint (it is {value!r})") from None
    if a.size == 0 or not bool(np.all((a >= 0.0) & np.isfinite(a) if finite else a >= 0.0)):
        raise ValueError(f"{name} must be >= 0 and " + ("finite" if finite else "not NaN (+inf is accepted)"))
    return a


def _broadcast_per_joint(a, J, name, config_name=None):
    """[J] contiguous float64 of `a` [1] or [J]; `config_name`: the constant of config that `a` is, when it is the default."""
    if a.shape not in ((1,), (J,)):
        raise ValueError(f"{name} must hold one value, or one per joint ({J})" + (f" (config.{config_name} is for 38)" if config_name else ""))
    return np.ascontiguousarray(np.broadcast_to(a, (J,)))


def _call(name, *args):
    """One entry of the library; its DF3D_EINVAL is the caller's mistake and becomes a ValueError with the library's message."""
    lib = _native.load()
    rc = getattr(lib, name)(*args)
    if rc == _native.DF3D_EINVAL:
        raise ValueError(lib.df3d_last_error().decode())
    _native.check(rc, name)


@_on_tensor_device
def heatmap_argmax(heatmaps, nonfinite=None, subpixel=False):
    """heatmaps [n, J, H, W] float32 (cuda) -> (points [n, J, 2] float32 (row/H, col/W), conf [n, J] float32).
    `nonfinite`: an int32 CUDA tensor of one element (zeroed by its owner) that is incremented once per plane holding an infinity or a NaN --
    the overflow guard of the reduced-precision engines (HourglassEngine.check_finite reads it).
    `subpixel=True` (df3d_heatmap_argmax_subpixel): the point is the arg-max cell moved by up to half a cell per axis to the
    maximum of the quadratic through its 3 x 3 neighbourhood; the cell, conf and the counter are those of the plain call."""
    lib = _native.load()
    _need(heatmaps, torch.float32, "heatmaps")
    n, j, h, w = heatmaps.shape
    pts = torch.empty((n, j, 2), dtype=torch.float32, device=heatmaps.device)
    conf = torch.empty((n, j), dtype=torch.float32, device=heatmaps.device)
    if nonfinite is not None and not (nonfinite.is_cuda and nonfinite.dtype == torch.int32 and nonfinite.numel() == 1 and nonfinite.device == heatmaps.device):
        raise ValueError("nonfinite must be a one-element int32 CUDA tensor on the heat-maps' device")
    name = "df3d_heatmap_argmax_subpixel" if subpixel else "df3d_heatmap_argmax_checked"
    _native.check(
        getattr(lib, name)(heatmaps.data_ptr(), n, j, h, w, pts.data_ptr(), conf.data_ptr(),
                           nonfinite.data_ptr() if nonfinite is not None else None, _stream(heatmaps)),
        name,
    )
    return pts, conf


@_on_tensor_device
def relayout_19_to_38(points19, camera_ordering):
    """points19 [7, T, 19, 2] float32 (cuda) -> [7, T, 38, 2] float64 (reference df3d/core.py:187-203)."""
    lib = _native.load()
    _need(points19, torch.float32, "points19")
    if points19.shape[0] != 7 or points19.shape[2] != 19 or points19.shape[3] != 2:
        raise ValueError("points19 must be [7, T, 19, 2]")
    T = points19.shape[1]
    order = (ctypes.c_int * 7)(*[int(c) for c in camera_ordering])
    out = torch.empty((7, T, 38, 2), dtype=torch.float64, device=points19.device)
    _native.check(lib.df3d_relayout_19_to_38(points19.data_ptr(), order, T, out.data_ptr(), _stream(points19)), "df3d_relayout_19_to_38")
    return out


@_on_tensor_device
def triangulate(P, points2d_px):
    """P [ncam, 3, 4] float64 (numpy or tensor), points2d_px [ncam, T, J, 2] float64 cuda (row_px, col_px)
    -> X [T, J, 3] float64 cuda; zeros where fewer than two cameras see the joint."""
    lib = _native.load()
    ncam, T, J = _need_points2d_px(points2d_px)
    Ph = _camera_matrices(P, ncam)
    X = torch.empty((T, J, 3), dtype=torch.float64, device=points2d_px.device)
    _native.check(
        lib.df3d_triangulate(Ph.ctypes.data_as(ctypes.c_void_p), points2d_px.data_ptr(), ncam, T, J, X.data_ptr(), _stream(points2d_px)),
        "df3d_triangulate",
    )
    return X


@_on_tensor_device
def column_median(cols):
    """cols [ncols, n] float64 cuda -> [ncols] exact medians (numpy.median semantics)."""
    lib = _native.load()
    _need(cols, torch.float64, "cols")
    ncols, n = cols.shape
    out = torch.empty((ncols,), dtype=torch.float64, device=cols.device)
    _native.check(lib.df3d_column_median(cols.data_ptr(), ncols, n, n, out.data_ptr(), _stream(cols)), "df3d_column_median")
    return out


@_on_tensor_device
def procrustes(points3d, tmpl_seg_med, tmpl_fit_med):
    """points3d [T, 38, 3] float64 cuda -> registered copy (a9).  tmpl_* are the template's host constants
    (deepfly3d_amd.procrustes.template_constants)."""
    lib = _native.load()
    _need(points3d, torch.float64, "points3d")
    if points3d.dim() != 3 or tuple(points3d.shape[1:]) != (38, 3):
        raise ValueError("points3d must be [T, 38, 3]")
    T = points3d.shape[0]
    seg = np.ascontiguousarray(tmpl_seg_med, dtype=np.float64)
    fit = np.ascontiguousarray(tmpl_fit_med, dtype=np.float64)
    if seg.shape != (2, 12) or fit.shape != (2, 6, 3):
        raise ValueError("template constants must be [2, 12] and [2, 6, 3]")
    need = lib.df3d_procrustes_work_doubles(T)
    work = torch.empty((need,), dtype=torch.float64, device=points3d.device)
    out = torch.empty_like(points3d)
    dp = ctypes.POINTER(ctypes.c_double)
    _native.check(
        lib.df3d_procrustes(points3d.data_ptr(), T, seg.ctypes.data_as(dp), fit.ctypes.data_as(dp), out.data_ptr(), work.data_ptr(), need,
                            _stream(points3d)),
        "df3d_procrustes",
    )
    return out


@_on_tensor_device
def pose_normalize(points3d, rotate=True):
    """[T, J, 3] float64 cuda -> minus the per-axis median of all points, optionally (x, y, z) -> (x, -z, -y)."""
    lib = _native.load()
    _need(points3d, torch.float64, "points3d")
    T, J, three = points3d.shape
    if three != 3:
        raise ValueError("points3d must be [T, J, 3]")
    work = torch.empty((1024,), dtype=torch.float64, device=points3d.device)   # medians + scratch of the long-column median
    out = torch.empty_like(points3d)
    _native.check(lib.df3d_pose_normalize(points3d.data_ptr(), T, J, 1 if rotate else 0, out.data_ptr(), work.data_ptr(), work.numel(), _stream(points3d)),
                  "df3d_pose_normalize")
    return out


@_on_tensor_device
def oneeuro_filter(series, freq=100.0, mincutoff=0.1, beta=2.0, dcutoff=1.0, first_stamp=1, stamp_step=0.1):
    """series [T, ...] float64 cuda: every trailing element is one channel filtered along T (reference
    df3d/signal_util.py:69-100 defaults)."""
    lib = _native.load()
    _need(series, torch.float64, "series")
    T = series.shape[0]
    nch = int(series[0].numel()) if T else 1
    out = torch.empty_like(series)
    _native.check(
        lib.df3d_oneeuro_filter(series.data_ptr(), T, nch, freq, mincutoff, beta, dcutoff, first_stamp, stamp_step, out.data_ptr(), _stream(series)),
        "df3d_oneeuro_filter",
    )
    return out


@_on_tensor_device
def heatmap_peaks(heatmaps, k, subpixel=False):
    """heatmaps [n, J, H, W] float32 (cuda) -> (count [n, J] int32, points [n, J, k, 2] float32 (row/H, col/W), values [n, J, k]
    float32): the k best local maxima of every plane (df3d_heatmap_peaks; peak 0 is heatmap_argmax's cell).  `subpixel=True`
    (df3d_heatmap_peaks_subpixel): the same peaks, every point refined as heatmap_argmax(subpixel=True) refines its own."""
    lib = _native.load()
    _need(heatmaps, torch.float32, "heatmaps")
    n, j, h, w = heatmaps.shape
    k = int(k)
    count = torch.empty((n, j), dtype=torch.int32, device=heatmaps.device)
    pts = torch.empty((n, j, k, 2), dtype=torch.float32, device=heatmaps.device)
    vals = torch.empty((n, j, k), dtype=torch.float32, device=heatmaps.device)
    name = "df3d_heatmap_peaks_subpixel" if subpixel else "df3d_heatmap_peaks"
    _native.check(getattr(lib, name)(heatmaps.data_ptr(), n, j, h, w, k, count.data_ptr(), pts.data_ptr(), vals.data_ptr(), _stream(heatmaps)), name)
    return count, pts, vals


def _pictorial_inputs(P, camera_ordering, points2d, peak_count, peak_pts, peak_val):
    _need(points2d, torch.float64, "points2d")
    _need(peak_count, torch.int32, "peak_count")
    _need(peak_pts, torch.float32, "peak_pts")
    if peak_val is not None:
        _need(peak_val, torch.float32, "peak_val")
    if points2d.dim() != 4 or points2d.shape[0] != 7 or tuple(points2d.shape[2:]) != (38, 2):
        raise ValueError("points2d must be [7, T, 38, 2]")
    T = points2d.shape[1]
    k = peak_pts.shape[3] if peak_pts.dim() == 5 else -1
    if tuple(peak_count.shape) != (7, T, 19) or tuple(peak_pts.shape) != (7, T, 19, k, 2) or (peak_val is not None and tuple(peak_val.shape) != (7, T, 19, k)):
        raise ValueError("peaks must be count [7, T, 19], points [7, T, 19, K, 2] and values [7, T, 19, K] of the recording of points2d")
    if any(t.device != points2d.device for t in (peak_count, peak_pts) + ((peak_val,) if peak_val is not None else ())):
        raise ValueError("points2d and the peaks must be on one device")
    order = (ctypes.c_int * 7)(*[int(c) for c in camera_ordering])
    return T, k, order, None if P is None else _camera_matrices(P, 7)


@_on_tensor_device
def ps_proposals(P, camera_ordering, points2d, peak_count, peak_pts, peak_val, image_shape, frames=None, num_proposals=64, tau=30.0,
                 w_reproj=1.0, w_heatmap=1.0, X0=None):
    """Proposals of the pictorial-structures model for frames [t0, t1) (default all), df3d_ps_proposals.  P [7, 3, 4] pixels of the
    physical cameras; points2d [7, T, 38, 2] float64 cuda (the re-layout of the arg-max detections, normalised); peaks as
    heatmap_peaks returns them per camera [7, T, 19, ...]; image_shape [W, H]; X0 = arg_max_points3d(P, points2d, image_shape), computed
    when None.  Returns {count [n, 38], index, X, U, match [n, 38, M]}."""
    lib = _native.load()
    T, k, order, Ph = _pictorial_inputs(P, camera_ordering, points2d, peak_count, peak_pts, peak_val)
    t0, t1 = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    n, m, dev = max(0, t1 - t0), int(num_proposals), points2d.device
    kept = {"count": torch.zeros((n, 38), dtype=torch.int32, device=dev), "index": torch.zeros((n, 38, max(m, 0)), dtype=torch.int32, device=dev),
            "X": torch.zeros((n, 38, max(m, 0), 3), dtype=torch.float64, device=dev), "U": torch.zeros((n, 38, max(m, 0)), dtype=torch.float64, device=dev),
            "match": torch.zeros((n, 38, max(m, 0)), dtype=torch.int32, device=dev)}
    dp = ctypes.POINTER(ctypes.c_double)
    if X0 is None:
        X0 = arg_max_points3d(Ph, points2d, image_shape)
    if tuple(X0.shape) != (T, 38, 3) or X0.dtype != torch.float64 or X0.device != dev or not X0.is_contiguous():
        raise ValueError("X0 must be the [T, 38, 3] float64 triangulation of points2d on its device")
    _native.check(
        lib.df3d_ps_proposals(Ph.ctypes.data_as(dp), order, X0.data_ptr(), peak_count.data_ptr(), peak_pts.data_ptr(), peak_val.data_ptr(), T, t0, t1 - t0,
                              k, m, float(image_shape[1]), float(image_shape[0]), float(tau), float(w_reproj), float(w_heatmap), kept["count"].data_ptr(),
                              kept["index"].data_ptr(), kept["X"].data_ptr(), kept["U"].data_ptr(), kept["match"].data_ptr(), _stream(points2d)),
        "df3d_ps_proposals",
    )
    return kept


@_on_tensor_device
def ps_solve(camera_ordering, points2d, peak_count, peak_pts, kept, frames=None, w_bone=1.0, out=None):
    """Exact min-sum over the skeleton's bone tree (config.bone_tree) on the kept proposals of frames [t0, t1), df3d_ps_solve.
    Writes those frames of out = (points2d [7, T, 38, 2], choice [T, 38] int32, energy [T] float64), allocated when None, and
    returns it."""
    from .config import bone_tree

    lib = _native.load()
    T, k, order, _ = _pictorial_inputs(None, camera_ordering, points2d, peak_count, peak_pts, None)
    t0, t1 = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    n, m, dev = max(0, t1 - t0), int(kept["index"].shape[-1]), points2d.device
    for name in ("count", "index", "X", "U", "match"):
        if kept[name].shape[:2] != (n, 38) or kept[name].device != dev:
            raise ValueError(f"kept[{name!r}] does not belong to frames [{t0}, {t1})")
    if out is None:
        out = (points2d.clone(), torch.zeros((T, 38), dtype=torch.int32, device=dev), torch.zeros((T,), dtype=torch.float64, device=dev))
    parent, bone = bone_tree()
    par = (ctypes.c_int * 38)(*[int(p) for p in parent])
    bone = np.ascontiguousarray(bone, dtype=np.float64)
    work = torch.empty((max(1, 38 * n),), dtype=torch.float64, device=dev)
    _native.check(
        lib.df3d_ps_solve(order, par, bone.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(w_bone), points2d.data_ptr(), peak_count.data_ptr(),
                          peak_pts.data_ptr(), T, t0, n, k, m, kept["count"].data_ptr(), kept["index"].data_ptr(), kept["X"].data_ptr(), kept["U"].data_ptr(),
                          kept["match"].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), work.data_ptr(), work.numel(), _stream(points2d)),
        "df3d_ps_solve",
    )
    return out


@_on_tensor_device
def arg_max_points3d(P, points2d, image_shape):
    """[T, 38, 3]: df3d_triangulate_scaled of the normalised points2d [7, T, 38, 2] (pixels = points2d * (H, W), as
    CameraNetwork.triangulate sees them) -- the correction's proposal 0, bit for bit what the uncorrected run triangulates."""
    lib = _native.load()
    _need(points2d, torch.float64, "points2d")
    ncam, T, J, _ = points2d.shape
    Ph = _camera_matrices(P, ncam)
    X = torch.empty((T, J, 3), dtype=torch.float64, device=points2d.device)
    _native.check(lib.df3d_triangulate_scaled(Ph.ctypes.data_as(ctypes.c_void_p), points2d.data_ptr(), float(image_shape[1]), float(image_shape[0]), ncam, T, J,
                                              X.data_ptr(), _stream(points2d)), "df3d_triangulate_scaled")
    return X


class PictorialResult:
    """What `pictorial_correct` returns (device tensors): points2d [7, T, 38, 2] float64 normalised (the corrected detections),
    choice [T, 38] int32 (the chosen proposal of every joint; 0 = the arg-max DLT), energy [T] float64 (each frame's minimum)."""

    def __init__(self, points2d, choice, energy):
        self.points2d, self.choice, self.energy = points2d, choice, energy


def pictorial_correct(P, camera_ordering, points2d, peak_count, peak_pts, peak_val, image_shape, num_proposals=64, tau=30.0, w_reproj=1.0,
                      w_heatmap=1.0, w_bone=1.0, chunk_frames=4096):
    """Pictorial-structures correction of the arg-max detections: proposals, then the exact solve, in chunks of
    `chunk_frames` frames so that the proposal storage stays bounded (~38 M 40 B per frame).  Arguments as ps_proposals."""
    T = points2d.shape[1]
    out = None
    chunk = max(1, int(chunk_frames))
    X0 = arg_max_points3d(P, points2d, image_shape) if T else None
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        kept = ps_proposals(P, camera_ordering, points2d, peak_count, peak_pts, peak_val, image_shape, (t0, t1), num_proposals, tau, w_reproj, w_heatmap, X0)
        out = ps_solve(camera_ordering, points2d, peak_count, peak_pts, kept, (t0, t1), w_bone, out)
    if out is None:   # an empty recording: validate the arguments all the same
        kept = ps_proposals(P, camera_ordering, points2d, peak_count, peak_pts, peak_val, image_shape, (0, 0), num_proposals, tau, w_reproj, w_heatmap)
        out = ps_solve(camera_ordering, points2d, peak_count, peak_pts, kept, (0, 0), w_bone, out)
    return PictorialResult(*out)


@_on_tensor_device
def reprojection_errors(P, points2d_px, X=None, thresholds=None, frames=None):
    """Per-joint reprojection errors and suspect-joint masks, df3d_reproj_errors.  P [ncam, 3, 4] float64
    (numpy or tensor, pixels); points2d_px [ncam, T, J, 2] float64 cuda (row_px, col_px); X [T, J, 3] float64 cuda on the same
    frames, triangulate() of the selected detections when None; thresholds [J] or [1] pixels (default config.REPROJ_THR, J = 38);
    frames: optional frame ids, gathered on the device from points2d_px (and X), the outputs in their order.
    Returns (err [ncam, nf, J], jmax [nf, J] float64, mask [nf] int64: bit j set when jmax > thresholds[j]) on the device."""
    from .config import REPROJ_THR

    lib = _native.load()
    ncam, T, J = _need_points2d_px(points2d_px)
    dev = points2d_px.device
    Ph = _camera_matrices(P, ncam)
    thr = np.ascontiguousarray(REPROJ_THR if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
    thr = _broadcast_per_joint(thr, J, "thresholds", "REPROJ_THR" if thresholds is None else None)
    if X is not None:
        _need_X(X, points2d_px)
    px = points2d_px
    if frames is not None:
        idx = torch.as_tensor(np.asarray(frames, dtype=np.int64).reshape(-1), device=dev)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= T):
            raise IndexError(f"frame ids must lie in [0, {T})")
        px = points2d_px.index_select(1, idx).contiguous()
        if X is not None:
            X = X.index_select(0, idx).contiguous()
    nf = px.shape[1]
    if X is None:
        X = triangulate(Ph, px)
    err = torch.empty((ncam, nf, J), dtype=torch.float64, device=dev)
    jmax = torch.empty((nf, J), dtype=torch.float64, device=dev)
    mask = torch.empty((nf,), dtype=torch.int64, device=dev)
    dp = ctypes.POINTER(ctypes.c_double)
    _native.check(
        lib.df3d_reproj_errors(Ph.ctypes.data_as(dp), px.data_ptr(), X.data_ptr(), ncam, nf, J, thr.ctypes.data_as(dp), err.data_ptr(), jmax.data_ptr(),
                               mask.data_ptr(), _stream(px)),
        "df3d_reproj_errors",
    )
    return err, jmax, mask


@_on_tensor_device
def body_frame(points3d):
    """points3d [n, 38, 3] float64 cuda -> [n, 3, 3]: rows ex, ey, ez of every pose's own body frame from its six body-coxa
    joints (df3d_body_frame); all NaN where one of them is missing or the six are degenerate."""
    lib = _native.load()
    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    n = points3d.shape[0]
    out = torch.empty((n, 3, 3), dtype=torch.float64, device=points3d.device)
    _native.check(lib.df3d_body_frame(points3d.data_ptr(), n, out.data_ptr(), _stream(points3d)), "df3d_body_frame")
    return out


def _coxa_medians(points3d):
    """(the six body-coxa joint ids, [6, 3] the exact temporal medians (column_median) of their 18 coordinates over all frames of
    points3d [T >= 1, 38, 3] as they stand)."""
    from .config import leg_joints

    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    coxae = torch.tensor([leg_joints(leg)[0] for leg in range(6)], device=points3d.device)
    cols = points3d.index_select(1, coxae).reshape(points3d.shape[0], 18).t().contiguous()   # the median wants contiguous columns
    return coxae, column_median(cols).reshape(6, 3)


def recording_frame(points3d):
    """[1, 3, 3]: the body frame of the pose whose 18 body-coxa coordinates are the temporal medians of those of points3d
    [T >= 1, 38, 3]: one frame for a tethered fly's recording."""
    coxae, medians = _coxa_medians(points3d)
    pose = torch.zeros((1, 38, 3), dtype=torch.float64, device=points3d.device)
    pose[0, coxae] = medians
    return body_frame(pose)


@_on_tensor_device
def joint_angles(points3d, body_frame="recording"):
    """Leg joint angles and segment lengths, df3d_joint_angles.  points3d [T, 38, 3] float64 cuda, the
    layout of points3d_wo_procrustes.  `body_frame`: "recording" (one frame for all poses, from the temporal medians of the six
    body-coxa joints), "per_frame" (every pose's own frame) or an explicit [3, 3] / [T, 3, 3] array or tensor (rows ex, ey, ez),
    used as given.  Returns (angles [T, 6, 8] radians in the order of config.LEG_ANGLE_NAMES, lengths [T, 6, 4]) on the device;
    NaN where a joint is missing or a direction is undefined."""
    lib = _native.load()
    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    T, dev = points3d.shape[0], points3d.device
    angles = torch.empty((T, 6, 8), dtype=torch.float64, device=dev)
    lengths = torch.empty((T, 6, 4), dtype=torch.float64, device=dev)
    frames = _body_frames(body_frame, T, dev)
    if T == 0:   # no medians to take, nothing to launch
        return angles, lengths
    frames = _fill_body_frames(frames, body_frame, points3d)
    _native.check(lib.df3d_joint_angles(points3d.data_ptr(), T, frames.data_ptr(), frames.shape[0], angles.data_ptr(), lengths.data_ptr(),
                                        _stream(points3d)), "df3d_joint_angles")
    return angles, lengths


@_on_tensor_device
def segment_length_medians(points3d):
    """points3d [T, 38, 3] float64 cuda -> [6, 4]: the median over the frames of every leg segment's length (coxa, femur, tibia,
    tarsus), the fixed lengths `fit_legs` uses by default.  The lengths are df3d_joint_angles' (they do not depend on the body
    frame); a frame in which an end joint is missing does not count, so each median is numpy.nanmedian's value, taken by
    column_median over the column's finite entries.  A segment without a finite length in any frame raises ValueError."""
    from .config import LEG_NAMES

    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    T, dev = points3d.shape[0], points3d.device
    names = ("coxa", "femur", "tibia", "tarsus")
    if T == 0:
        raise ValueError(f"leg 0 ({LEG_NAMES[0]}), segment 0 (coxa) has no finite length in any frame: there are no frames")
    lengths = joint_angles(points3d, torch.eye(3, dtype=torch.float64, device=dev))[1]
    cols = lengths.reshape(T, 24).t().contiguous()
    finite = torch.isfinite(cols)
    counts = finite.sum(dim=1).cpu()
    if int(counts.min()) == T:
        return column_median(cols).reshape(6, 4)
    out = torch.empty((24,), dtype=torch.float64, device=dev)
    for c in range(24):   # columns of different heights: one median each
        if int(counts[c]) == 0:
            raise ValueError(f"leg {c // 4} ({LEG_NAMES[c // 4]}), segment {c % 4} ({names[c % 4]}) has no finite length in any frame")
        out[c] = column_median(cols[c][finite[c]].reshape(1, -1).contiguous())[0]
    return out.reshape(6, 4)


class LegFitResult:
    """What `fit_legs` returns: points [T, 38, 3] float64 (the pose with every fitted leg replaced by its constant-length chain),
    cost [T, 6] float64 (each leg's summed squared distance from the measured joints, NaN where the leg was not fitted),
    status [T, 6] and iters [T, 6] int32 (0 converged, 1 max_iter reached, 2 the damping ran out, -1 not fitted; accepted
    iterations, -1 where not fitted) -- device tensors -- and lengths [6, 4], the fixed lengths as used (a host numpy array)."""

    def __init__(self, points, cost, status, iters, lengths):
        self.points, self.cost, self.status, self.iters, self.lengths = points, cost, status, iters, lengths


def _leg_table(value, shape, name):
    """A host float64 array of `shape` from an array or tensor."""
    a = value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
    if a.shape != shape or a.dtype.kind not in "fiu":
        raise ValueError(f"an explicit {name} must be a numeric {list(shape)} array")
    return np.ascontiguousarray(a, dtype=np.float64)


@_on_tensor_device
def fit_legs(points3d, lengths="recording", anchor="per_frame", max_iter=None):
    """Fit a chain of constant segment lengths to every leg of every pose, df3d_leg_fit.  points3d
    [T, 38, 3] float64 cuda, the layout of points3d_wo_procrustes.  `lengths`: "recording" (segment_length_medians(points3d)) or a
    [6, 4] array.  `anchor`: "per_frame" (each leg starts at its own measured body-coxa joint), "recording" (at the temporal
    median of that joint, one point per leg for the whole recording) or a [6, 3] array.  `max_iter` defaults to
    config.RIGID_LEGS_MAX_ITER; 0 replays the measured directions with the fixed lengths.  Returns a LegFitResult; the input is
    not changed, and the eight joints that belong to no leg are copied."""
    from .config import RIGID_LEGS_MAX_ITER

    max_iter = RIGID_LEGS_MAX_ITER if max_iter is None else int(max_iter)
    if max_iter < 0:
        raise ValueError("max_iter must be >= 0")
    if isinstance(lengths, str) and lengths != "recording":
        raise ValueError('lengths must be "recording" or a [6, 4] array')
    if isinstance(anchor, str) and anchor not in ("per_frame", "recording"):
        raise ValueError('anchor must be "per_frame", "recording" or a [6, 3] array')
    table = None if isinstance(lengths, str) else _leg_table(lengths, (6, 4), "lengths")
    origin = None if isinstance(anchor, str) else _leg_table(anchor, (6, 3), "anchor")
    lib = _native.load()
    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    T, dev = points3d.shape[0], points3d.device
    if table is None:
        table = np.ascontiguousarray(segment_length_medians(points3d).cpu().numpy())
    if isinstance(anchor, str) and anchor == "recording":
        if T == 0:
            raise ValueError('anchor="recording" needs at least one frame to take the medians of')
        origin = np.ascontiguousarray(_coxa_medians(points3d)[1].cpu().numpy())
    out = points3d.clone()
    cost = torch.empty((T, 6), dtype=torch.float64, device=dev)
    info = torch.empty((T, 6, 2), dtype=torch.int32, device=dev)
    as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    _native.check(lib.df3d_leg_fit(points3d.data_ptr(), T, as_ptr(table), None if origin is None else as_ptr(origin), max_iter,
                                   out.data_ptr(), cost.data_ptr(), info.data_ptr(), _stream(points3d)), "df3d_leg_fit")
    return LegFitResult(out, cost, info[..., 0], info[..., 1], table)


def wavelet_frequencies(fps, f_min=None, f_max=None, num=None):
    """[num] float64 (numpy): the bank's frequencies f_i = f_min (f_max / f_min)^(i / (num - 1)) in Hz, geometric from f_min to
    f_max; num = 1 gives f_min.  Defaults (config): f_min = SPECTROGRAM_F_MIN, f_max = fps * SPECTROGRAM_F_MAX_OVER_FPS,
    num = SPECTROGRAM_NUM_FREQS.  f_max may be raised to fps / 2, where the negative-frequency image of a real series folds into
    the row."""
    from . import config

    fps = float(fps)
    f_min = config.SPECTROGRAM_F_MIN if f_min is None else float(f_min)
    f_max = fps * config.SPECTROGRAM_F_MAX_OVER_FPS if f_max is None else float(f_max)
    num = config.SPECTROGRAM_NUM_FREQS if num is None else int(num)
    if not (np.isfinite(fps) and fps > 0):
        raise ValueError("fps must be finite and > 0")
    if not (np.isfinite(f_min) and f_min > 0):
        raise ValueError("f_min must be finite and > 0")
    if not 1 <= num <= 64:
        raise ValueError("num must be in [1, 64]")
    if not f_max >= f_min:
        raise ValueError(f"f_max ({f_max:g}) must not be below f_min ({f_min:g})")
    if not f_max <= fps / 2:
        raise ValueError(f"f_max ({f_max:g}) must be at most fps / 2 ({fps / 2:g})")
    if num == 1:
        return np.array([f_min], dtype=np.float64)
    freqs = f_min * (f_max / f_min) ** (np.arange(num, dtype=np.float64) / (num - 1))
    freqs[-1] = f_max   # the power rounds: the last row is f_max itself, so that f_max = fps / 2 stays admissible
    return freqs


def _wavelet_bank(fps, freqs, omega0, radius):
    """(fps, freqs [F] contiguous float64 numpy, omega0, radius, the workspace's bytes) with the defaults filled in, refused by the
    library's own rules (ValueError with its message) before a device is touched."""
    from . import config

    fps = float(fps)
    omega0 = config.SPECTROGRAM_OMEGA0 if omega0 is None else float(omega0)
    radius = config.SPECTROGRAM_RADIUS if radius is None else float(radius)
    if freqs is None:
        freqs = wavelet_frequencies(fps)
    freqs = freqs.detach().cpu().numpy() if isinstance(freqs, torch.Tensor) else np.asarray(freqs)
    if freqs.ndim != 1 or freqs.dtype.kind not in "fiu":
        raise ValueError("freqs must be a numeric [F] array")
    freqs = np.ascontiguousarray(freqs, dtype=np.float64)
    need = _workspace("df3d_spectrogram_work_bytes", freqs.ctypes.data_as(ctypes.c_void_p), freqs.shape[0], fps, omega0, radius, device=None)[1]
    return fps, freqs, omega0, radius, need


def wavelet_support(fps, freqs=None, omega0=None, radius=None):
    """[F] int64 (numpy): K_i = ceil(radius omega0 fps / (2 pi f_i)), the half support of every row in samples.  Row i of
    wavelet_spectrogram at time t reads the samples t - K_i .. t + K_i: within K_i of either end it leans on the edge extension."""
    fps, freqs, omega0, radius, _ = _wavelet_bank(fps, freqs, omega0, radius)
    return np.ceil(radius * (omega0 * fps / (2.0 * np.pi * freqs))).astype(np.int64)


@_on_tensor_device
def wavelet_spectrogram(series, fps, freqs=None, omega0=None, radius=None, dtype=torch.float64):
    """Morlet wavelet amplitudes of every channel of a bundle of time series, df3d_spectrogram.  series
    [T], [T, C] or [T, ...] float64 cuda, time first; the trailing axes are flattened and restored, so [T, 6, 8] gives
    [T, 6, 8, F].  `fps` the sampling rate in Hz; `freqs` the rows' frequencies (default wavelet_frequencies(fps)); `omega0`,
    `radius` default to config's.  Returns [T, ..., F] of `dtype` (torch.float64, or torch.float32: accumulated in float64 and
    rounded once) on the series' device and stream: an amplitude in the units of the series, the ends extended by their edge
    value, NaN exactly where a sample within K_i (wavelet_support) of the time is not finite."""
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    fps, freqs, omega0, radius, need = _wavelet_bank(fps, freqs, omega0, radius)
    if not (isinstance(series, torch.Tensor) and series.is_cuda and series.dtype == torch.float64 and series.dim() >= 1):
        raise ValueError("series must be a torch.float64 CUDA tensor of shape [T, ...]")
    lib = _native.load()
    T, shape, F, dev = series.shape[0], tuple(series.shape), freqs.shape[0], series.device
    C = int(np.prod(shape[1:], dtype=np.int64))
    if C < 1:
        raise ValueError("series must hold at least one channel")
    x = series.reshape(T, C).t().contiguous()   # [C, T]: a block reads one channel's run of times
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = torch.empty((T, C, F), dtype=dtype, device=dev)
    fp, stream = freqs.ctypes.data_as(ctypes.c_void_p), _stream(series)
    _native.check(lib.df3d_spectrogram_bank(fp, F, fps, omega0, radius, work.data_ptr(), need, stream), "df3d_spectrogram_bank")
    _native.check(lib.df3d_spectrogram(x.data_ptr(), T, C, fp, F, fps, omega0, radius, work.data_ptr(), need, out.data_ptr(),
                                       int(dtype == torch.float32), stream), "df3d_spectrogram")
    return out.reshape(*shape, F)


def unwrap_phase(series, channels=None):
    """numpy.unwrap's rule along time on the device: series [T, C] float64 (any device), `channels` the columns to unwrap (a
    list of indices; default all).  Every step between consecutive samples is brought into [-pi, pi] by a multiple of 2 pi (a
    step of exactly -pi that came from a positive difference becomes +pi; a step whose size is below pi is left alone) and the
    corrections are summed up.  A requested column that holds a non-finite sample is left as it is.  Returns (the unwrapped
    copy, the list of the columns left for that reason)."""
    if not (isinstance(series, torch.Tensor) and series.dtype == torch.float64 and series.dim() == 2):
        raise ValueError("series must be a torch.float64 tensor of shape [T, C]")
    T, C = series.shape
    cols = list(range(C)) if channels is None else [int(c) for c in channels]
    if any(not 0 <= c < C for c in cols):
        raise ValueError(f"channels must lie in [0, {C})")
    out = series.clone()
    if T < 2 or not cols:
        return out, []
    idx = torch.tensor(cols, device=series.device)
    p = series.index_select(1, idx)
    finite = torch.isfinite(p).all(dim=0)
    d = p[1:] - p[:-1]
    m = torch.remainder(d + np.pi, 2.0 * np.pi) - np.pi
    m = torch.where((m == -np.pi) & (d > 0), torch.full_like(m, np.pi), m)
    corr = torch.where(d.abs() < np.pi, torch.zeros_like(d), m - d)
    up = p.clone()
    up[1:] += torch.cumsum(corr, dim=0)
    out[:, idx] = torch.where(finite.unsqueeze(0), up, p)
    return out, [c for c, ok in zip(cols, finite.cpu().tolist()) if not ok]


# ---- t-SNE behaviour maps of per-frame spectra ---------------------------------------------------------------
BehaviourMapResult = collections.namedtuple("BehaviourMapResult", "embedding train_index beta info kl perplexity")


def _need_f64(t, dims, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() in dims):
        raise ValueError(f"{name} must be a torch.float64 CUDA tensor of {' or '.join(str(d) for d in dims)} dimensions")
    return t.contiguous()


def behaviour_map_points(frames, perplexity=None, max_points=None):
    """(N, perplexity): how many of `frames` valid frames a behaviour map embeds, N = min(frames, max_points), after the model's
    refusals (ValueError): max_points outside [1, config.BEHAVIOUR_POINTS_CAP]; a perplexity that is not finite or <= 1; fewer
    frames than 3 perplexity + 1 -- every training frame calibrates against the N - 1 others, and the rule is 3 perplexity <= N - 1."""
    from . import config

    u = float(config.BEHAVIOUR_PERPLEXITY if perplexity is None else perplexity)
    cap = config.BEHAVIOUR_POINTS_CAP
    max_points = int(config.BEHAVIOUR_MAX_POINTS if max_points is None else max_points)
    if not 1 <= max_points <= cap:
        raise ValueError(f"max_points must be in [1, {cap}] (it is {max_points}): the dense N x N float64 tables are 2 GB each at {cap}")
    if not (np.isfinite(u) and u > 1.0):
        raise ValueError(f"perplexity must be finite and > 1 (it is {u:g})")
    N = min(int(frames), max_points)
    need = int(np.ceil(3.0 * u)) + 1
    if N < need:
        what = f"this recording has {int(frames)} valid frames" if int(frames) <= max_points else f"max_points is {max_points}"
        raise ValueError(f"perplexity {u:g} needs at least {need} frames to embed (3 perplexity <= frames - 1) and {what}: "
                         f"the largest perplexity accepted for {N} frames is {max((N - 1) / 3.0, 0.0):.4g}")
    return N, u


def behaviour_train_rows(valid_count, N):
    """[N] int64 (numpy): the positions floor(i valid_count / N), i = 0..N - 1, of the training frames in the list of valid frames."""
    return (np.arange(N, dtype=np.int64) * int(valid_count)) // max(int(N), 1)


def _distributions(S):
    """(p [T, D], log p [T, D], e [T], valid [T] int32) of S [T, ...]: df3d_bmap_prepare."""
    from . import config

    if not (isinstance(S, torch.Tensor) and S.is_cuda and S.dtype == torch.float64 and S.dim() >= 1):
        raise ValueError("S must be a torch.float64 CUDA tensor of shape [T, ...]")
    T = S.shape[0]
    D = int(np.prod(tuple(S.shape[1:]), dtype=np.int64))
    if D < 1:
        raise ValueError("S must hold at least one channel")
    S2 = S.reshape(T, D).contiguous()
    p, logp = torch.empty_like(S2), torch.empty_like(S2)
    e = torch.empty((T,), dtype=torch.float64, device=S.device)
    valid = torch.empty((T,), dtype=torch.int32, device=S.device)
    _call("df3d_bmap_prepare", S2.data_ptr(), T, D, config.BEHAVIOUR_FLOOR, p.data_ptr(), logp.data_ptr(), e.data_ptr(), valid.data_ptr(),
          _stream(S))
    return p, logp, e, valid


@_on_tensor_device
def spectrogram_distributions(S):
    """(p [T, D] float64, valid [T] bool): every frame's spectrum S[t] (non-negative amplitudes; [T, ...], the trailing axes
    flattened to D) as a distribution over its channels, p = (S / sum S + floor) / (1 + D floor) with floor =
    config.BEHAVIOUR_FLOOR.  A row with a negative or non-finite entry or a zero sum is not valid; its p is NaN."""
    p, _, _, valid = _distributions(S)
    return p, valid != 0


def _divergence(pa, ea, lb):
    M, D = pa.shape
    N = lb.shape[0]
    K = torch.empty((M, N), dtype=torch.float64, device=pa.device)
    step = 65535 * 128   # the most rows one call takes
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        _call("df3d_bmap_divergence", pa[m0:m1].data_ptr(), ea[m0:m1].data_ptr(), m1 - m0, lb.data_ptr(), N, D, K[m0:m1].data_ptr(), _stream(pa))
    return K


def _logs(p):
    logp = torch.empty_like(p)
    e = torch.empty((p.shape[0],), dtype=torch.float64, device=p.device)
    _call("df3d_bmap_logs", p.data_ptr(), p.shape[0], p.shape[1], logp.data_ptr(), e.data_ptr(), _stream(p))
    return logp, e


@_on_tensor_device
def kl_divergence(pa, pb):
    """K [M, N] float64: K[i, j] = max(0, sum_d pa[i, d] (log pa[i, d] - log pb[j, d])), the Kullback-Leibler divergence of row i
    of pa [M, D] from row j of pb [N, D] (distributions with positive entries, as spectrogram_distributions gives them).  The
    matrix is not symmetric."""
    pa, pb = _need_f64(pa, (2,), "pa"), _need_f64(pb, (2,), "pb")
    if pa.shape[1] != pb.shape[1] or pa.shape[1] < 1 or pa.device != pb.device:
        raise ValueError("pa [M, D] and pb [N, D] must share D >= 1 and the device")
    return _divergence(pa, _logs(pa)[1], _logs(pb)[0])


@_on_tensor_device
def perplexity_calibrate(K, perplexity=None, exclude=None):
    """(cond [M, N], beta [M], info [M] int32) of a divergence table K [M, N]: cond[i] = softmax_j(-beta_i K[i, j]) with beta_i chosen
    so that the row's entropy is log(perplexity) to config.BEHAVIOUR_ENTROPY_TOL nats.  `exclude`: None (every column takes
    part), "self" (column i of row i is left out and gets 0; K must be square) or an int32 tensor [M] of the column each row
    leaves out (-1: none).  A row in which at least `perplexity` entries tie at the minimum cannot reach the target: it gets
    beta = config.BEHAVIOUR_BETA_MAX and bit 0 of its info.  ValueError: a perplexity that is not finite, <= 1 or above a third
    of the admitted columns."""
    from . import config

    K = _need_f64(K, (2,), "K")
    M, N = K.shape
    u = float(config.BEHAVIOUR_PERPLEXITY if perplexity is None else perplexity)
    if isinstance(exclude, str):
        if exclude != "self" or M != N:
            raise ValueError('exclude must be None, "self" (K square) or an int32 tensor [M]')
        exclude = torch.arange(M, dtype=torch.int32, device=K.device)
    elif exclude is not None:
        if not (isinstance(exclude, torch.Tensor) and exclude.dtype == torch.int32 and exclude.shape == (M,) and exclude.device == K.device):
            raise ValueError('exclude must be None, "self" (K square) or an int32 tensor [M] on the device of K')
        exclude = exclude.contiguous()
    cond = torch.empty_like(K)
    beta = torch.empty((M,), dtype=torch.float64, device=K.device)
    info = torch.empty((M,), dtype=torch.int32, device=K.device)
    _call("df3d_bmap_calibrate", K.data_ptr(), M, N, u, config.BEHAVIOUR_ENTROPY_TOL, config.BEHAVIOUR_BETA_MAX,
          None if exclude is None else exclude.data_ptr(), cond.data_ptr(), beta.data_ptr(), info.data_ptr(), _stream(K))
    return cond, beta, info


@_on_tensor_device
def joint_probabilities(cond):
    """P [N, N] = (cond + cond^T) / (2N) with a zero diagonal: the joint table of the training set."""
    cond = _need_f64(cond, (2,), "cond")
    if cond.shape[0] != cond.shape[1]:
        raise ValueError("cond must be square")
    P = torch.empty_like(cond)
    _call("df3d_bmap_joint", cond.data_ptr(), cond.shape[0], P.data_ptr(), _stream(cond))
    return P


_TSNE_REFUSAL = "N must be in [1, {}] (it is {{}})"   # df3d_bmap_work_bytes': the cap is config.BEHAVIOUR_POINTS_CAP, then N


@_on_tensor_device
def tsne(P, init, n_iter=None, first_iter=0, state=None):
    """(Y, V, G), each [N, 2]: iterations first_iter .. first_iter + n_iter - 1 (default config.BEHAVIOUR_ITERATIONS) of the
    model's descent on the joint table P [N, N] from the positions `init` [N, 2] and `state` = (V, G) (default: V = 0, G = 1, the
    start).  The step size is max(N / 48, 50); the exaggeration and the momentum follow the absolute iteration index, so a run may
    be split anywhere and resumed from what it returned.  Nothing is read back."""
    from . import config

    P, Y = _need_f64(P, (2,), "P"), _need_f64(init, (2,), "init").clone()
    N = P.shape[0]
    if P.shape != (N, N) or Y.shape != (N, 2) or Y.device != P.device:
        raise ValueError("P must be [N, N] and init [N, 2] on its device")
    n_iter = config.BEHAVIOUR_ITERATIONS if n_iter is None else int(n_iter)
    if state is None:
        V, G = torch.zeros_like(Y), torch.ones_like(Y)
    else:
        V, G = (_need_f64(t, (2,), "state").clone() for t in state)
        if V.shape != Y.shape or G.shape != Y.shape:
            raise ValueError("state must be (V [N, 2], G [N, 2])")
    if N == 0:
        return Y, V, G
    work, need = _workspace("df3d_bmap_work_bytes", N, device=P.device, refusal=_TSNE_REFUSAL.format(config.BEHAVIOUR_POINTS_CAP))
    _call("df3d_tsne_run", P.data_ptr(), N, Y.data_ptr(), V.data_ptr(), G.data_ptr(), int(first_iter), n_iter, max(N / 48.0, 50.0),
          work.data_ptr(), need, _stream(P))
    return Y, V, G


@_on_tensor_device
def tsne_cost(P, Y):
    """The Kullback-Leibler cost sum_{P_ij > 0} P_ij log(P_ij Z / w_ij) of the positions Y [N, 2] under the joint table P [N, N]:
    a float64 tensor of one element on the device (nothing is read back)."""
    from . import config

    P, Y = _need_f64(P, (2,), "P"), _need_f64(Y, (2,), "Y")
    N = P.shape[0]
    if P.shape != (N, N) or Y.shape != (N, 2) or Y.device != P.device:
        raise ValueError("P must be [N, N] and Y [N, 2] on its device")
    work, need = _workspace("df3d_bmap_work_bytes", N, device=P.device, refusal=_TSNE_REFUSAL.format(config.BEHAVIOUR_POINTS_CAP))
    cost = torch.empty((1,), dtype=torch.float64, device=P.device)
    _call("df3d_bmap_cost", P.data_ptr(), N, Y.data_ptr(), cost.data_ptr(), work.data_ptr(), need, _stream(P))
    return cost[0]


_PLACE_CHUNK_BYTES = 1 << 28   # the most bytes of one row chunk's divergence table during placement


@_on_tensor_device
def behaviour_map(S, perplexity=None, n_iter=None, max_points=None, seed=0):
    """The t-SNE behaviour map of per-frame spectra S [T, ...] (float64 cuda, non-negative), a
    BehaviourMapResult: `embedding` [T, 2] (NaN for a frame that is not valid), `train_index` [N] int64 (the frames that were
    embedded by descent, N = min(valid frames, max_points), spread evenly over the valid ones; every other valid frame is placed
    at the mean of the training positions under its own calibrated conditional), `beta` [T] and `info` [T] int32 (the
    calibration's, NaN / 0 for an invalid frame; bit 0: the perplexity could not be met, the frame's neighbours tie), `kl` (the
    final cost, a float, the one value read back) and `perplexity`.  Defaults: config.BEHAVIOUR_PERPLEXITY, _ITERATIONS,
    _MAX_POINTS; the start is 1e-4 times standard normals of a CPU torch.Generator seeded with `seed`."""
    if not (isinstance(S, torch.Tensor) and S.dim() >= 1):
        raise ValueError("S must be a torch.float64 CUDA tensor of shape [T, ...]")
    T, dev = S.shape[0], S.device
    behaviour_map_points(T, perplexity, max_points)   # too few frames whatever their validity: refused before any work
    p, logp, e, valid = _distributions(S)
    vidx = torch.nonzero(valid).flatten()
    Tv = int(vidx.numel())
    N, u = behaviour_map_points(Tv, perplexity, max_points)
    rows = torch.from_numpy(behaviour_train_rows(Tv, N)).to(dev)
    train = vidx[rows]
    pt, lt, et = p[train], logp[train], e[train]
    cond, beta_t, info_t = perplexity_calibrate(_divergence(pt, et, lt), u, "self")
    P = joint_probabilities(cond)
    del cond
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    Y0 = (1e-4 * torch.randn((N, 2), generator=gen, dtype=torch.float64)).to(dev)
    Y = tsne(P, Y0, n_iter)[0]
    kl = tsne_cost(P, Y)
    del P
    embedding = torch.full((T, 2), float("nan"), dtype=torch.float64, device=dev)
    beta = torch.full((T,), float("nan"), dtype=torch.float64, device=dev)
    info = torch.zeros((T,), dtype=torch.int32, device=dev)
    embedding[train], beta[train], info[train] = Y, beta_t, info_t
    placed = torch.ones((Tv,), dtype=torch.bool, device=dev)
    placed[rows] = False
    rest = vidx[placed]
    chunk = max(1, _PLACE_CHUNK_BYTES // (8 * N))
    for r0 in range(0, int(rest.numel()), chunk):   # row chunks: no [T, N] table ever exists
        sel = rest[r0 : r0 + chunk]
        c, b, i = perplexity_calibrate(_divergence(p[sel], e[sel], lt), u)
        out = torch.empty((sel.numel(), 2), dtype=torch.float64, device=dev)
        _call("df3d_bmap_place", c.data_ptr(), sel.numel(), N, Y.data_ptr(), out.data_ptr(), _stream(S))
        embedding[sel], beta[sel], info[sel] = out, b, i
    return BehaviourMapResult(embedding, train, beta, info, float(kl.item()), u)


# ---- segmentation of the behaviour map -------------------------------------------------------------------------
BehaviourSegmentsResult = collections.namedtuple("BehaviourSegmentsResult",
                                                 "density origin sigma regions region_peaks labels bouts occupancy transitions")


_BSEG_REFUSAL = "no workspace for T = {} frames on a grid of {}: grid must be in [2, 1024] and T at most 65 535 * 2 048"   # df3d_bseg_work_bytes'


def _need_grid(grid):
    from . import config

    return _integer(config.BEHAVIOUR_GRID if grid is None else grid, *config.BEHAVIOUR_GRID_RANGE, "grid")


def density_grid(lo, hi, grid=None, sigma=None):
    """((x0, y0, h), sigma): the square grid of the model over a map whose valid rows span lo = (min x, min y) .. hi = (max x,
    max y).  ext = max(hi - lo), c = (lo + hi) / 2, sigma = `sigma` or config.BEHAVIOUR_DENSITY_SIGMA_FRACTION ext, L = ext / 2 +
    3 sigma, x0 = c_x - L, y0 = c_y - L, h = 2 L / grid.  ValueError: a sigma that is not finite and > 0 -- among them the default of
    a map without extent."""
    from . import config

    G = _need_grid(grid)
    lo, hi = (float(lo[0]), float(lo[1])), (float(hi[0]), float(hi[1]))
    ext = max(hi[0] - lo[0], hi[1] - lo[1])
    if sigma is None:
        if not ext > 0.0:
            raise ValueError("every valid frame of the map lies on one point, so the default sigma (a fraction of the map's extent) is 0: "
                             "give sigma")
        sigma = config.BEHAVIOUR_DENSITY_SIGMA_FRACTION * ext
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma must be finite and > 0 (it is {sigma:g})")
    L = ext / 2.0 + 3.0 * sigma
    x0, y0 = (lo[0] + hi[0]) / 2.0 - L, (lo[1] + hi[1]) / 2.0 - L
    h = 2.0 * L / G
    if not (np.isfinite(h) and h > 0.0 and np.isfinite(x0) and np.isfinite(y0)):
        raise ValueError(f"the map's extent {ext:g} and sigma {sigma:g} leave no finite grid")
    return (x0, y0, h), sigma


@_on_tensor_device
def map_density(Y, grid=None, sigma=None):
    """(rho [G, G] float64, (x0, y0, h), sigma): the Gaussian density of the map Y [T, 2] (float64 cuda; a row with a non-finite
    entry is not valid and contributes nothing) on the grid density_grid() lays over its valid rows: rho[r, q] = (M 2 pi sigma^2)^-1
    sum_t exp(-|g_rq - Y[t]|^2 / (2 sigma^2)) with g_rq = (x0 + (q + 0.5) h, y0 + (r + 0.5) h), the exact sum over all M valid frames.
    `grid`: G, default config.BEHAVIOUR_GRID.  The five bounds are read back.  ValueError: no valid row, and density_grid's."""
    Y = _need_tensor(Y, torch.float64, (2,), "Y")
    G = _need_grid(grid)
    T = Y.shape[0]
    bounds = torch.zeros((5,), dtype=torch.float64, device=Y.device)
    _call("df3d_bseg_bounds", Y.data_ptr(), T, bounds.data_ptr(), _stream(Y))
    b = bounds.cpu().tolist()
    if T == 0 or b[4] < 1.0:
        raise ValueError(f"the map holds no valid frame ({T} rows, each with a non-finite entry): there is nothing to take a density of")
    origin, sigma = density_grid((b[0], b[2]), (b[1], b[3]), G, sigma)
    rho = torch.empty((G, G), dtype=torch.float64, device=Y.device)
    work, need = _workspace("df3d_bseg_work_bytes", T, G, device=Y.device, refusal=_BSEG_REFUSAL)
    _call("df3d_bseg_density", Y.data_ptr(), T, origin[0], origin[1], origin[2], G, sigma, rho.data_ptr(), work.data_ptr(), need, _stream(Y))
    return rho, origin, sigma


@_on_tensor_device
def watershed(rho, min_peak=None):
    """(regions [G, G] int32, root_cells [R] int32) of a density rho [G, G] (float64 cuda, finite, >= 0): every cell climbs to the
    8-neighbour with the largest key (rho, -index) until none is larger (index = r G + q: among equal densities the smaller index
    is the higher, so plateaux and an all-equal field are decided); the peaks with rho > 0 and rho >= min_peak max rho (default
    config.BEHAVIOUR_MIN_PEAK, in [0, 1]) found the regions 1 .. R, numbered by rising index; a cell whose peak was dropped is 0.
    `root_cells`: the peaks' indices.  R is read back."""
    from . import config

    rho = _need_f64(rho, (2,), "rho")
    G = rho.shape[0]
    if rho.shape != (G, G):
        raise ValueError("rho must be square, [G, G]")
    _need_grid(G)
    min_peak = float(config.BEHAVIOUR_MIN_PEAK if min_peak is None else min_peak)
    if not 0.0 <= min_peak <= 1.0:
        raise ValueError(f"min_peak must be in [0, 1] (it is {min_peak:g})")
    regions = torch.empty((G, G), dtype=torch.int32, device=rho.device)
    roots = torch.empty((G * G,), dtype=torch.int32, device=rho.device)
    count = torch.empty((1,), dtype=torch.int32, device=rho.device)
    work, need = _workspace("df3d_bseg_work_bytes", 0, G, device=rho.device, refusal=_BSEG_REFUSAL)
    _call("df3d_bseg_watershed", rho.data_ptr(), G, min_peak, regions.data_ptr(), count.data_ptr(), roots.data_ptr(), work.data_ptr(), need,
          _stream(rho))
    return regions, roots[: int(count.item())].clone()


@_on_tensor_device
def map_labels(Y, regions, origin):
    """labels [T] int32: -1 for a row of Y [T, 2] with a non-finite entry, else regions[r, q] of the cell the frame lies in,
    q = clamp(floor((Y[t, 0] - x0) / h), 0, G - 1) and r likewise from Y[t, 1] and y0; origin = (x0, y0, h)."""
    Y = _need_tensor(Y, torch.float64, (2,), "Y")
    if not (isinstance(regions, torch.Tensor) and regions.is_cuda and regions.dtype == torch.int32 and regions.dim() == 2
            and regions.shape[0] == regions.shape[1] and regions.device == Y.device):
        raise ValueError("regions must be a torch.int32 CUDA tensor of shape [G, G] on the device of Y")
    G = _need_grid(regions.shape[0])
    x0, y0, h = (float(v) for v in origin)
    regions = regions.contiguous()
    labels = torch.empty((Y.shape[0],), dtype=torch.int32, device=Y.device)
    _call("df3d_bseg_labels", Y.data_ptr(), Y.shape[0], x0, y0, h, G, regions.data_ptr(), labels.data_ptr(), _stream(Y))
    return labels


@_on_tensor_device
def ethogram(labels, num_regions):
    """(bouts [B, 3] int64, occupancy [R + 1] int64, transitions [R + 1, R + 1] int64) of labels [T] (int32 cuda, -1 .. R =
    num_regions): the maximal runs of equal labels as rows (label, start, length) -- runs of -1 and of 0 among them, their lengths
    sum to T --, the frames of each label 0 .. R, and the counts of pairs (t, t + 1) whose labels are both >= 0 and differ.  B is
    read back."""
    labels = _need_tensor(labels, torch.int32, (), "labels")
    R = int(num_regions)
    if not 0 <= R <= 32767:
        raise ValueError(f"num_regions must be in [0, 32767] (it is {R})")
    T, dev = labels.shape[0], labels.device
    occupancy = torch.zeros((R + 1,), dtype=torch.int64, device=dev)
    transitions = torch.zeros((R + 1, R + 1), dtype=torch.int64, device=dev)
    if T == 0:
        return torch.zeros((0, 3), dtype=torch.int64, device=dev), occupancy, transitions
    bouts = torch.empty((T, 3), dtype=torch.int64, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    work, need = _workspace("df3d_bseg_work_bytes", T, 2, device=dev, refusal=_BSEG_REFUSAL)
    _call("df3d_bseg_bouts", labels.data_ptr(), T, R, bouts.data_ptr(), count.data_ptr(), occupancy.data_ptr(), transitions.data_ptr(),
          work.data_ptr(), need, _stream(labels))
    return bouts[: int(count.item())].clone(), occupancy, transitions


@_on_tensor_device
def segment_map(Y, grid=None, sigma=None, min_peak=None):
    """The segmentation of a behaviour map Y [T, 2] (float64 cuda), a BehaviourSegmentsResult: `density`
    [G, G], `origin` (x0, y0, h) and `sigma` (map_density), `regions` [G, G] int32 (watershed), `region_peaks` [R, 2] float64 (the
    map coordinates of the centres of the peaks' cells), `labels` [T] int32 (map_labels), and `bouts`, `occupancy`, `transitions`
    (ethogram)."""
    rho, origin, sigma = map_density(Y, grid, sigma)
    regions, roots = watershed(rho, min_peak)
    G = rho.shape[0]
    r, q = torch.div(roots, G, rounding_mode="floor"), roots % G
    peaks = torch.stack((origin[0] + (q.double() + 0.5) * origin[2], origin[1] + (r.double() + 0.5) * origin[2]), dim=1)
    labels = map_labels(Y, regions, origin)
    bouts, occupancy, transitions = ethogram(labels, roots.numel())
    return BehaviourSegmentsResult(rho, origin, sigma, regions, peaks, labels, bouts, occupancy, transitions)


# ---- gait analysis of the leg tips ---------------------------------------------------------------------------
@dataclasses.dataclass
class GaitResult:
    """What `gait` returns, device tensors but for the last two: tip, vel [T, 6, 3] float64 (tip_kinematics), states [T, 6] int32
    (gait_states), steps [S, 4] int64 and step_metrics [S, 3] float64 (gait_steps), phase [T, 6] float64 (gait_phase), coupling
    [6, 6, 2] float64 and coupling_count [6, 6] int64 (gait_coupling), pattern [T] int32, pattern_histogram [64] and state_counts
    [6, 3] int64 (gait_patterns), thresholds (on, off, half_window) and fps."""
    tip: torch.Tensor
    vel: torch.Tensor
    states: torch.Tensor
    steps: torch.Tensor
    step_metrics: torch.Tensor
    phase: torch.Tensor
    coupling: torch.Tensor
    coupling_count: torch.Tensor
    pattern: torch.Tensor
    pattern_histogram: torch.Tensor
    state_counts: torch.Tensor
    thresholds: tuple
    fps: float


_LEGS_REFUSAL = "no workspace for T = {} frames: T must be at most (2^31 - 1) / 6"   # df3d_gait_work_bytes' and df3d_ball_work_bytes'


def _gait_fps(fps):
    return _number(fps, "fps", positive=True)


def gait_thresholds(on=None, off=None, half_window=None):
    """(on, off, half_window) with config.GAIT_SWING_ON, GAIT_SWING_OFF and GAIT_DIFF_HALF for what is None.  ValueError: a threshold
    that is not finite, on <= off, a half window that is no integer in config.GAIT_DIFF_HALF_RANGE."""
    from . import config

    on = float(config.GAIT_SWING_ON if on is None else on)
    off = float(config.GAIT_SWING_OFF if off is None else off)
    if not (np.isfinite(on) and np.isfinite(off)):
        raise ValueError(f"on and off must be finite (they are {on:g} and {off:g})")
    if not on > off:
        raise ValueError(f"on must be above off (they are {on:g} and {off:g})")
    return on, off, _integer(config.GAIT_DIFF_HALF if half_window is None else half_window, *config.GAIT_DIFF_HALF_RANGE, "half_window")


@_on_tensor_device
def tip_kinematics(points3d, fps, body_frame="recording", half_window=None):
    """(tip, vel), both [T, 6, 3] float64, of points3d [T, 38, 3] (float64 cuda, the layout of points3d_wo_procrustes) sampled at
    `fps`: every leg's tip relative to its body-coxa joint, q(P4 - P0), and the tip's velocity q(P4[b] - P4[a]) fps / (b - a) over
    the window a = max(t - half_window, 0), b = min(t + half_window, T - 1), in the leg coordinates of joint_angles (x anterior,
    side-1 legs mirrored in y) and pose units (per second).  `body_frame` as in joint_angles.  NaN where an end joint is missing
    (the velocity: P4 at a or at b), where the window is empty (T = 1) or where the frame holds a non-finite number."""
    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    fps, w = _gait_fps(fps), gait_thresholds(half_window=half_window)[2]
    T, dev = points3d.shape[0], points3d.device
    tip = torch.empty((T, 6, 3), dtype=torch.float64, device=dev)
    vel = torch.empty((T, 6, 3), dtype=torch.float64, device=dev)
    frames = _body_frames(body_frame, T, dev)
    if T == 0:
        return tip, vel
    frames = _fill_body_frames(frames, body_frame, points3d)
    _call("df3d_gait_velocity", points3d.data_ptr(), T, frames.data_ptr(), frames.shape[0], fps, w, tip.data_ptr(), vel.data_ptr(),
          _stream(points3d))
    return tip, vel


@_on_tensor_device
def gait_states(vel, on=None, off=None):
    """states [T, 6] int32 of vel [T, 6, 3] (float64 cuda, tip_kinematics'): swing/stance by hysteresis on the anterior velocity
    u = vel[..., 0].  A sample is unknown where u is NaN, swing where u > on, stance where u < off (defaults config.GAIT_SWING_ON and
    GAIT_SWING_OFF, a guess nobody has measured on a recording) and keeps the state otherwise; the state is that of the last
    deciding sample at or before t: -1 unknown, 0 stance, 1 swing, and -1 before the first."""
    vel = _need_tensor(vel, torch.float64, (6, 3), "vel")
    on, off, _ = gait_thresholds(on, off)
    T = vel.shape[0]
    states = torch.empty((T, 6), dtype=torch.int32, device=vel.device)
    if T:
        work, need = _workspace("df3d_gait_work_bytes", T, device=vel.device, refusal=_LEGS_REFUSAL)
        _call("df3d_gait_states", vel.data_ptr(), T, on, off, states.data_ptr(), work.data_ptr(), need, _stream(vel))
    return states


@_on_tensor_device
def gait_steps(states, tip, fps):
    """(steps [S, 4] int64, metrics [S, 3] float64) of states [T, 6] (int32 cuda) and tip [T, 6, 3]: a lift-off is a frame t >= 1
    with states 0 then 1, a touch-down the reverse; a step is a pair of consecutive lift-offs t0 < t2 of a leg with no unknown
    state in [t0, t2], and t1 the one touch-down between them.  Rows (leg, t0, t1, t2) ordered by (leg, t0); metrics: swing duration
    (t1 - t0) / fps, stance duration (t2 - t1) / fps, stride tip[t1, leg, 0] - tip[t0, leg, 0] (NaN where either tip is).  S is
    read back."""
    states = _need_tensor(states, torch.int32, (6,), "states")
    tip = _need_tensor(tip, torch.float64, (6, 3), "tip")
    fps = _gait_fps(fps)
    T, dev = states.shape[0], states.device
    if tip.shape[0] != T or tip.device != dev:
        raise ValueError(f"tip must hold the {T} frames of states, on their device")
    if T == 0:
        return torch.zeros((0, 4), dtype=torch.int64, device=dev), torch.zeros((0, 3), dtype=torch.float64, device=dev)
    steps = torch.empty((3 * T, 4), dtype=torch.int64, device=dev)
    metrics = torch.empty((3 * T, 3), dtype=torch.float64, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    work, need = _workspace("df3d_gait_work_bytes", T, device=dev, refusal=_LEGS_REFUSAL)
    _call("df3d_gait_steps", states.data_ptr(), tip.data_ptr(), T, fps, steps.data_ptr(), metrics.data_ptr(), count.data_ptr(),
          work.data_ptr(), need, _stream(states))
    S = int(count.item())
    return steps[:S].clone(), metrics[:S].clone()


@_on_tensor_device
def gait_phase(states):
    """phase [T, 6] float64 of states [T, 6] (int32 cuda): (t - t0) / (t2 - t0) for the step of the leg with t0 <= t < t2
    (gait_steps), NaN outside every step."""
    states = _need_tensor(states, torch.int32, (6,), "states")
    T = states.shape[0]
    phase = torch.empty((T, 6), dtype=torch.float64, device=states.device)
    if T:
        work, need = _workspace("df3d_gait_work_bytes", T, device=states.device, refusal=_LEGS_REFUSAL)
        _call("df3d_gait_phase", states.data_ptr(), T, phase.data_ptr(), work.data_ptr(), need, _stream(states))
    return phase


@_on_tensor_device
def gait_coupling(phase):
    """(mean [6, 6, 2] float64, count [6, 6] int64) of phase [T, 6] (float64 cuda): for every ordered pair of legs the mean of
    (cos, sin)(2 pi (phase_i - phase_j)) over the count[i, j] frames where both phases are finite, NaN where there is none.  The
    resultant length is numpy.hypot of the two components and the mean angle their arctan2."""
    phase = _need_tensor(phase, torch.float64, (6,), "phase")
    T, dev = phase.shape[0], phase.device
    mean = torch.full((6, 6, 2), float("nan"), dtype=torch.float64, device=dev)
    count = torch.zeros((6, 6), dtype=torch.int64, device=dev)
    if T:
        work, need = _workspace("df3d_gait_work_bytes", T, device=dev, refusal=_LEGS_REFUSAL)
        _call("df3d_gait_coupling", phase.data_ptr(), T, mean.data_ptr(), count.data_ptr(), work.data_ptr(), need, _stream(phase))
    return mean, count


@_on_tensor_device
def gait_patterns(states):
    """(pattern [T] int32, histogram [64] int64, state_counts [6, 3] int64) of states [T, 6] (int32 cuda): every frame's mask of
    the legs in swing (bit L = leg L; config.GAIT_TRIPODS are the two tripods), -1 where a leg is unknown; the frames of every
    mask; every leg's unknown, stance and swing frames."""
    states = _need_tensor(states, torch.int32, (6,), "states")
    T, dev = states.shape[0], states.device
    pattern = torch.empty((T,), dtype=torch.int32, device=dev)
    histogram = torch.zeros((64,), dtype=torch.int64, device=dev)
    counts = torch.zeros((6, 3), dtype=torch.int64, device=dev)
    if T:
        _call("df3d_gait_patterns", states.data_ptr(), T, pattern.data_ptr(), histogram.data_ptr(), counts.data_ptr(), _stream(states))
    return pattern, histogram, counts


def gait(points3d, fps, body_frame="recording", on=None, off=None, half_window=None):
    """The gait analysis of points3d [T, 38, 3] (float64 cuda) sampled at `fps`, a GaitResult: tip_kinematics,
    gait_states, gait_steps, gait_phase, gait_coupling and gait_patterns, each on the one before."""
    thresholds = gait_thresholds(on, off, half_window)   # refused before any work
    fps = _gait_fps(fps)
    tip, vel = tip_kinematics(points3d, fps, body_frame, thresholds[2])
    states = gait_states(vel, thresholds[0], thresholds[1])
    steps, metrics = gait_steps(states, tip, fps)
    phase = gait_phase(states)
    mean, count = gait_coupling(phase)
    pattern, histogram, counts = gait_patterns(states)
    return GaitResult(tip, vel, states, steps, metrics, phase, mean, count, pattern, histogram, counts, thresholds, fps)


# ---- the treadmill ball and the fictive walking path --------------------------------------------------------
@dataclasses.dataclass
class BallFit:
    """What `fit_ball` returns, device tensors that nothing reads back: ball [8] float64 (centre, radius, rms and three zeros, the
    layout df3d_ball_rotation reads), info [2] int64 (count, status) and sums [17] float64 (the folded slice sums of the algebraic
    fit, include/df3d_hip.h).  center, radius, rms, count and status are views of them.  status bit 0: the fit was refused (centre,
    radius and rms NaN); bit 1: a known-radius fit without an algebraic centre, started beyond the tips' mean."""
    ball: torch.Tensor
    info: torch.Tensor
    sums: torch.Tensor

    center = property(lambda self: self.ball[:3])
    radius = property(lambda self: self.ball[3])
    rms = property(lambda self: self.ball[4])
    count = property(lambda self: self.info[0])
    status = property(lambda self: self.info[1])


@dataclasses.dataclass
class TreadmillResult:
    """What `treadmill` returns, device tensors but for the last two: tip, vel [T, 6, 3] float64 (body_tips), states [T, 6] int32, ball
    (a BallFit), rotation [T, 3] float64 (rad/s, body coordinates), legs [T] int32, residual [T] and fictive [T, 3] (forward mm/s,
    sideways mm/s, yaw rad/s; ball_rotation), path [T, 3] (x, y, theta) and skipped (a 0-dim int64 tensor; fictive_path), params
    (radius or NaN, on, off, half_window, min_legs, iterations; on and off NaN where the states were handed in) and fps."""
    tip: torch.Tensor
    vel: torch.Tensor
    states: torch.Tensor
    ball: BallFit
    rotation: torch.Tensor
    legs: torch.Tensor
    residual: torch.Tensor
    fictive: torch.Tensor
    path: torch.Tensor
    skipped: torch.Tensor
    params: tuple
    fps: float


def treadmill_params(radius=None, min_legs=None, iterations=None):
    """(radius or None, min_legs, iterations) with config.BALL_MIN_LEGS and BALL_FIT_ITERATIONS for what is None -- guesses nobody has
    measured on a recording.  ValueError: a radius that is no finite number > 0, a min_legs that is no integer in
    config.BALL_MIN_LEGS_RANGE, iterations that are no integer in config.BALL_FIT_ITERATIONS_RANGE."""
    from . import config

    if radius is not None:
        radius = _number(radius, "radius", positive=True)
    min_legs = _integer(config.BALL_MIN_LEGS if min_legs is None else min_legs, *config.BALL_MIN_LEGS_RANGE, "min_legs")
    iterations = _integer(config.BALL_FIT_ITERATIONS if iterations is None else iterations, *config.BALL_FIT_ITERATIONS_RANGE, "iterations")
    return radius, min_legs, iterations


def _same_frames(t, T, dev, name):
    if t.shape[0] != T or t.device != dev:
        raise ValueError(f"{name} must hold the {T} frames of tips, on their device")


@_on_tensor_device
def body_tips(points3d, fps, body_frame="recording", half_window=None):
    """(tips, vel), both [T, 6, 3] float64, of points3d [T, 38, 3] (float64 cuda, the layout of points3d_wo_procrustes) sampled at
    `fps`: every leg's tip in the recording's body frame, F (P4 - o) with o the mean of the six body-coxa temporal medians -- neither
    mirrored nor relative to the coxa, unlike tip_kinematics -- and its velocity F (P4[b] - P4[a]) fps / (b - a) over gait's window.
    `body_frame`: "recording" or an explicit [3, 3] array or tensor (rows ex, ey, ez).  NaN where the tip is missing (the velocity: at
    a or at b), where the window is empty (T = 1) or where the frame or o holds a non-finite number."""
    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    fps, w = _gait_fps(fps), gait_thresholds(half_window=half_window)[2]
    T, dev = points3d.shape[0], points3d.device
    frame = _body_frames(body_frame, T, dev, per_frame_allowed=False,
                         text=('body_frame must be "recording" or a [3, 3] array: the ball is one object in one frame',
                               "an explicit body_frame must be [3, 3]: the ball is one object in one frame"))
    tips = torch.empty((T, 6, 3), dtype=torch.float64, device=dev)
    vel = torch.empty((T, 6, 3), dtype=torch.float64, device=dev)
    if T == 0:
        return tips, vel
    coxa = _coxa_medians(points3d)[1].contiguous()
    frame = _fill_body_frames(frame, body_frame, points3d)   # [1, 3, 3]: the nine numbers df3d_ball_tips reads
    _call("df3d_ball_tips", points3d.data_ptr(), T, frame.data_ptr(), coxa.data_ptr(), fps, w, tips.data_ptr(), vel.data_ptr(),
          _stream(points3d))
    return tips, vel


@_on_tensor_device
def fit_ball(tips, states, radius=None, iterations=None):
    """The sphere through the stance tips, a BallFit: tips [T, 6, 3] (float64 cuda, body_tips') and states [T, 6] (int32 cuda,
    gait_states'); a sample is a (t, L) with states 0 and a finite tip.  `radius=None`: the algebraic (Kasa) fit on coordinates
    centred at the samples' mean -- its radius is biased low by noise.  A known `radius` (pose units, mm): the centre takes
    `iterations` (config.BALL_FIT_ITERATIONS) Gauss-Newton steps on sum (|tip - c| - radius)^2 from the algebraic centre.  Refused
    (NaN, status bit 0): fewer than 4 samples (3 with a known radius) or a pivot at or below config.BALL_PIVOT_MIN times the largest
    diagonal entry.  Nothing is read back."""
    from . import config

    tips = _need_tensor(tips, torch.float64, (6, 3), "tips")
    states = _need_tensor(states, torch.int32, (6,), "states")
    radius, _, iterations = treadmill_params(radius, None, iterations)
    T, dev = tips.shape[0], tips.device
    _same_frames(states, T, dev, "states")
    ball = torch.full((8,), float("nan"), dtype=torch.float64, device=dev)
    ball[5:] = 0.0
    info = torch.tensor([0, 1], dtype=torch.int64, device=dev)   # no frames: no samples, a refused fit
    sums = torch.zeros((17,), dtype=torch.float64, device=dev)
    if T:
        work, need = _workspace("df3d_ball_work_bytes", T, device=dev, refusal=_LEGS_REFUSAL)
        _call("df3d_ball_fit", tips.data_ptr(), states.data_ptr(), T, 0 if radius is None else 1, 0.0 if radius is None else radius,
              iterations, float(config.BALL_PIVOT_MIN), ball.data_ptr(), info.data_ptr(), sums.data_ptr(), work.data_ptr(), need,
              _stream(tips))
    return BallFit(ball, info, sums)


@_on_tensor_device
def ball_rotation(tips, vel, states, ball, min_legs=None):
    """(rotation [T, 3], legs [T] int32, residual [T], fictive [T, 3]) of tips and vel [T, 6, 3] (body_tips'), states [T, 6] and `ball`
    (a BallFit, or its [8] float64 tensor: centre, radius, ...): per frame the rotation vector of the ball (rad/s, body coordinates)
    that best carries the stance tips, r = tip - c, sum (|r|^2 I - r r^T) omega = sum r x vel over the legs with states 0 and finite
    tip and vel; NaN with fewer than `min_legs` of them (config.BALL_MIN_LEGS), with a pivot at or below config.BALL_FRAME_PIVOT_MIN
    times the trace, or with a refused ball.  residual: the root mean square of vel - omega x r; fictive: the fly's forward and
    sideways speed (pose units per second) and yaw rate (rad/s)."""
    from . import config

    tips = _need_tensor(tips, torch.float64, (6, 3), "tips")
    vel = _need_tensor(vel, torch.float64, (6, 3), "vel")
    states = _need_tensor(states, torch.int32, (6,), "states")
    min_legs = treadmill_params(None, min_legs)[1]
    T, dev = tips.shape[0], tips.device
    _same_frames(vel, T, dev, "vel")
    _same_frames(states, T, dev, "states")
    ball = ball.ball if isinstance(ball, BallFit) else ball
    if not (isinstance(ball, torch.Tensor) and ball.dtype == torch.float64 and ball.device == dev and tuple(ball.shape) == (8,)):
        raise ValueError("ball must be a BallFit or its torch.float64 tensor of shape [8] on the device of tips")
    ball = ball.contiguous()
    rotation = torch.empty((T, 3), dtype=torch.float64, device=dev)
    legs = torch.empty((T,), dtype=torch.int32, device=dev)
    residual = torch.empty((T,), dtype=torch.float64, device=dev)
    fictive = torch.empty((T, 3), dtype=torch.float64, device=dev)
    if T:
        _call("df3d_ball_rotation", tips.data_ptr(), vel.data_ptr(), states.data_ptr(), T, ball.data_ptr(), min_legs,
              float(config.BALL_FRAME_PIVOT_MIN), rotation.data_ptr(), legs.data_ptr(), residual.data_ptr(), fictive.data_ptr(),
              _stream(tips))
    return rotation, legs, residual, fictive


@_on_tensor_device
def fictive_path(fictive, fps):
    """(path [T, 3] float64 = (x, y, theta), skipped, a 0-dim int64 tensor) of fictive [T, 3] (float64 cuda, ball_rotation's) sampled at
    `fps`: theta_0 = 0, theta_{t+1} = theta_t + yaw_t / fps; (x, y)_0 = 0, (x, y)_{t+1} = (x, y)_t + Rot(theta_t)(forward_t,
    sideways_t) / fps.  A frame with a non-finite component moves nothing and is counted in `skipped`."""
    fictive = _need_tensor(fictive, torch.float64, (3,), "fictive")
    fps = _gait_fps(fps)
    T, dev = fictive.shape[0], fictive.device
    path = torch.empty((T, 3), dtype=torch.float64, device=dev)
    skipped = torch.zeros((1,), dtype=torch.int64, device=dev)
    if T:
        work, need = _workspace("df3d_ball_work_bytes", T, device=dev, refusal=_LEGS_REFUSAL)
        _call("df3d_ball_path", fictive.data_ptr(), T, fps, path.data_ptr(), skipped.data_ptr(), work.data_ptr(), need, _stream(fictive))
    return path, skipped[0]


def treadmill(points3d, fps, body_frame="recording", states=None, radius=None, on=None, off=None, half_window=None, min_legs=None,
              iterations=None):
    """The treadmill analysis of points3d [T, 38, 3] (float64 cuda) sampled at `fps`, a TreadmillResult:
    body_tips, fit_ball over the stance samples, ball_rotation and fictive_path, each on the one before.  `states`: the swing/stance
    states [T, 6] of gait_states, handed in by whoever has them; None computes them from the anterior tip velocity with gait's
    rule and `on`, `off` (gait_thresholds).  `radius`: the ball's known radius in pose units (mm), else it is fitted."""
    radius, min_legs, iterations = treadmill_params(radius, min_legs, iterations)   # refused before any work
    thresholds = gait_thresholds(on, off, half_window)
    if states is not None and (on is not None or off is not None):
        raise ValueError("on and off decide the states that treadmill computes: with states handed in they have nothing to decide")
    fps = _gait_fps(fps)
    tip, vel = body_tips(points3d, fps, body_frame, thresholds[2])
    if states is None:
        states = gait_states(vel, thresholds[0], thresholds[1])   # the anterior velocity is tip_kinematics' own: F (P4[b] - P4[a]) . ex
        on, off = thresholds[:2]
    else:
        states = _need_tensor(states, torch.int32, (6,), "states")
        _same_frames(states, tip.shape[0], tip.device, "states")
        on = off = float("nan")
    ball = fit_ball(tip, states, radius, iterations)
    rotation, legs, residual, fictive = ball_rotation(tip, vel, states, ball, min_legs)
    path, skipped = fictive_path(fictive, fps)
    params = (float("nan") if radius is None else radius, on, off, thresholds[2], min_legs, iterations)
    return TreadmillResult(tip, vel, states, ball, rotation, legs, residual, fictive, path, skipped, params, fps)


# ---- repair of the 3-D pose ---------------------------------------------------------------------------------
@dataclasses.dataclass
class PoseRepairResult:
    """What `repair_pose` returns, device tensors but for the last: points [T, 38, 3] float64 (the repaired pose), status [T, 38] int8
    (0 kept, 1 missing and filled, 2 outlier and filled, 3 missing and left, 4 outlier and removed), counts [38, 5] int64 (the frames
    per joint and code), score [T, 38] float64 (the largest dev / threshold over the coordinates, NaN for a missing or untested joint)
    and params (half_window, threshold, floor, max_gap, min_count)."""
    points: torch.Tensor
    status: torch.Tensor
    counts: torch.Tensor
    score: torch.Tensor
    params: tuple


def repair_params(half_window=None, threshold=None, floor=None, max_gap=None, min_count=None):
    """(half_window, threshold, floor, max_gap, min_count) with config.REPAIR_HALF_WINDOW, REPAIR_THRESHOLD, REPAIR_FLOOR,
    REPAIR_MAX_GAP and REPAIR_MIN_COUNT for what is None -- guesses nobody has measured on a recording.  ValueError: a half window that
    is no integer in config.REPAIR_HALF_WINDOW_RANGE, a threshold that is not finite and > 0, a floor that is not finite and >= 0, a
    max_gap that is no integer in config.REPAIR_MAX_GAP_RANGE, a min_count that is no integer in [1, 2 half_window + 1]."""
    from . import config

    h = _integer(config.REPAIR_HALF_WINDOW if half_window is None else half_window, *config.REPAIR_HALF_WINDOW_RANGE, "half_window")
    k = _number(config.REPAIR_THRESHOLD if threshold is None else threshold, "threshold")
    if not (np.isfinite(k) and k > 0.0):
        raise ValueError(f"threshold must be finite and > 0 (it is {k:g})")
    fl = _number(config.REPAIR_FLOOR if floor is None else floor, "floor")
    if not (np.isfinite(fl) and fl >= 0.0):
        raise ValueError(f"floor must be finite and >= 0 (it is {fl:g})")
    gap = _integer(config.REPAIR_MAX_GAP if max_gap is None else max_gap, *config.REPAIR_MAX_GAP_RANGE, "max_gap")
    n_min = _integer(config.REPAIR_MIN_COUNT if min_count is None else min_count, 1, 2 * h + 1, "min_count")
    return h, k, fl, gap, n_min


@_on_tensor_device
def pose_outliers(points3d, half_window=None, threshold=None, floor=None, min_count=None):
    """(flags [T, 38] uint8, score [T, 38] float64) of points3d [T, 38, 3] (float64 cuda, the layout of points3d_wo_procrustes): a
    Hampel test of every joint, one pass.  flags: bit 0 = the joint is missing (a non-finite coordinate, or all three 0), bit 1 = it
    is an outlier: in some coordinate it lies further from the median of the valid frames of [t - half_window, t + half_window] than
    max(threshold * 1.4826 * their median absolute deviation, floor).  A window with fewer than min_count valid frames is not tested.
    score: the largest deviation / bound over the coordinates, NaN for a missing or untested joint.  Defaults: repair_params."""
    from . import config

    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    h, k, fl, _, n_min = repair_params(half_window, threshold, floor, None, min_count)
    T, dev = points3d.shape[0], points3d.device
    flags = torch.empty((T, 38), dtype=torch.uint8, device=dev)
    score = torch.empty((T, 38), dtype=torch.float64, device=dev)
    if T:
        _call("df3d_repair_outliers", points3d.data_ptr(), T, h, k * config.REPAIR_MAD_TO_SIGMA, fl, n_min, flags.data_ptr(),
              score.data_ptr(), _stream(points3d))
    return flags, score


@_on_tensor_device
def fill_gaps(points3d, flags, max_gap=None):
    """(points [T, 38, 3] float64, status [T, 38] int8, counts [38, 5] int64) of points3d [T, 38, 3] (float64 cuda) and flags [T, 38]
    (uint8 cuda, pose_outliers'): a joint whose flags are not 0 is interpolated linearly between its last good frame before and its
    first good frame after, where both exist and at most max_gap frames lie between them, and set to 0 -- missing -- otherwise.  Good
    joints keep their bits; nothing is extrapolated.  status: 0 kept, 1 missing and filled, 2 outlier and filled, 3 missing and left,
    4 outlier and removed; counts: the frames per joint and code."""
    points3d = _need_tensor(points3d, torch.float64, (38, 3), "points3d")
    T, dev = points3d.shape[0], points3d.device
    if not (isinstance(flags, torch.Tensor) and flags.dtype == torch.uint8 and flags.device == dev and tuple(flags.shape) == (T, 38)):
        raise ValueError(f"flags must be a torch.uint8 tensor of shape [{T}, 38] on the device of points3d")
    flags = flags.contiguous()
    gap = repair_params(max_gap=max_gap)[3]
    points = torch.empty_like(points3d)
    status = torch.empty((T, 38), dtype=torch.int8, device=dev)
    counts = torch.zeros((38, 5), dtype=torch.int64, device=dev)
    if T:
        work, need = _workspace("df3d_repair_work_bytes", T, device=dev, refusal="no workspace for T = {} frames: T must be at most (2^31 - 1) / 38")
        _call("df3d_repair_fill", points3d.data_ptr(), flags.data_ptr(), T, gap, points.data_ptr(), status.data_ptr(), counts.data_ptr(),
              work.data_ptr(), need, _stream(points3d))
    return points, status, counts


def repair_pose(points3d, half_window=None, threshold=None, floor=None, max_gap=None, min_count=None):
    """The repaired pose of points3d [T, 38, 3] (float64 cuda), a PoseRepairResult: pose_outliers, then
    fill_gaps of its flags."""
    params = repair_params(half_window, threshold, floor, max_gap, min_count)   # refused before any work
    flags, score = pose_outliers(points3d, params[0], params[1], params[2], params[4])
    points, status, counts = fill_gaps(points3d, flags, params[3])
    return PoseRepairResult(points, status, counts, score, params)


# ---- tracking of the 2-D detections through time ------------------------------------------------------------
@dataclasses.dataclass
class TrackResult:
    """What `track_peaks` returns, device tensors but for the last: choice [C, T, J] int32 (the slot of every frame on the jointly best
    sequence of its chain; 0 on a frame without a valid peak), cost [C, J] int64 (the minimum, in units of 2^-20; `cost_float` divides)
    and params (tau, w_motion, w_value, block_frames)."""
    choice: torch.Tensor
    cost: torch.Tensor
    params: tuple

    @property
    def cost_float(self):
        return self.cost.to(torch.float64) / 2.0 ** 20


def track_params(tau=None, w_motion=None, w_value=None, block_frames=None):
    """(tau, w_motion, w_value, block_frames) with config.TRACK_DEFAULTS for what is None -- tau and the weights are guesses nobody has
    measured on a recording.  ValueError: a tau that is not finite and > 0, a weight that is not finite or outside [0,
    config.TRACK_WEIGHT_MAX], a block_frames that is no integer in config.TRACK_BLOCK_FRAMES_RANGE."""
    from . import config

    d = config.TRACK_DEFAULTS
    t = _number(d["tau"] if tau is None else tau, "tau")
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError(f"tau must be finite and > 0 (it is {t:g})")
    weights = []
    for name, v in (("w_motion", w_motion), ("w_value", w_value)):
        w = _number(d[name] if v is None else v, name)
        if not (np.isfinite(w) and 0.0 <= w <= config.TRACK_WEIGHT_MAX):
            raise ValueError(f"{name} must be finite and in [0, {config.TRACK_WEIGHT_MAX:g}] (it is {w:g})")
        weights.append(w)
    b = _integer(d["block_frames"] if block_frames is None else block_frames, *config.TRACK_BLOCK_FRAMES_RANGE, "block_frames")
    return t, weights[0], weights[1], b


def _need_peaks(peak_count, peak_pts, peak_val):
    """(C, T, J, K) of count [C, T, J] int32, points [C, T, J, K, 2] float32 and values [C, T, J, K] float32 on one CUDA device."""
    from . import config

    _need(peak_count, torch.int32, "peak_count")
    _need(peak_pts, torch.float32, "peak_pts")
    _need(peak_val, torch.float32, "peak_val")
    if peak_count.dim() != 3 or peak_pts.dim() != 5 or tuple(peak_pts.shape[:3]) != tuple(peak_count.shape) or peak_pts.shape[4] != 2 or \
            tuple(peak_val.shape) != tuple(peak_pts.shape[:4]):
        raise ValueError("peaks must be count [C, T, J], points [C, T, J, K, 2] and values [C, T, J, K]")
    if peak_pts.device != peak_count.device or peak_val.device != peak_count.device:
        raise ValueError("the peaks must be on one device")
    C, T, J, K = peak_val.shape
    lo, hi = config.TRACK_NUM_PEAKS_RANGE
    if not lo <= K <= hi:
        raise ValueError(f"the peaks kept per heat-map, K, must be in [{lo}, {hi}] (it is {K})")
    if C < 1 or J < 1:
        raise ValueError("the peaks must hold at least one camera and one joint")
    return C, T, J, K


@_on_tensor_device
def track_peaks(peak_count, peak_pts, peak_val, image_shape, tau=None, w_motion=None, w_value=None, block_frames=None):
    """The jointly best sequence of heat-map peaks of every chain (camera, joint) over the recording (df3d_track_peaks, DESIGN.md section
    22), a TrackResult.  Peaks as heatmap_peaks returns them per camera: count [C, T, J] int32, points [C, T, J, K, 2] float32, values
    [C, T, J, K] float32 (cuda); image_shape [W, H].  A path pays w_value min(v_best - v, 1) for a peak whose value lies below the
    frame's best and w_motion min(|jump|^2, tau^2) / tau^2 for the jump from the peak of the frame before, in pixels; costs are quantised
    to multiples of 2^-20 and the solve is exact, so the result does not depend on block_frames.  Defaults and refusals: track_params."""
    t, wm, wv, b = track_params(tau, w_motion, w_value, block_frames)   # refused before any device work
    C, T, J, K = _need_peaks(peak_count, peak_pts, peak_val)
    W, H = float(image_shape[0]), float(image_shape[1])
    dev = peak_count.device
    choice = torch.empty((C, T, J), dtype=torch.int32, device=dev)
    cost = torch.zeros((C, J), dtype=torch.int64, device=dev)
    if T:
        work, need = _workspace("df3d_track_work_bytes", C * J, T, K, b, device=dev,
                                refusal="no workspace for {} chains of {} frames: C J must be at most 2^20, T at most 2^31 - 1 and C J T at most 2^36")
        _call("df3d_track_peaks", peak_count.data_ptr(), peak_pts.data_ptr(), peak_val.data_ptr(), C, T, J, K, H, W, t, wm, wv, b,
              choice.data_ptr(), cost.data_ptr(), work.data_ptr(), need, _stream(peak_count))
    return TrackResult(choice, cost, (t, wm, wv, b))


def tracked_points2d(points2d, camera_ordering, peak_pts, choice):
    """[7, T, 38, 2] float64: points2d [7, T, 38, 2] (float64 cuda, the re-layout of the arg-max detections) with every entry whose chain
    chose another slot than 0 replaced by the chosen peak of peak_pts [7, T, 19, K, 2], passed through relayout_19_to_38 -- flip and
    layout follow that one rule.  An entry whose chain chose slot 0 (a frame without a valid peak included), and every entry no chain
    fills, keeps its bits.  choice [7, T, 19] int32 (TrackResult.choice)."""
    _need(points2d, torch.float64, "points2d")
    _need(peak_pts, torch.float32, "peak_pts")
    _need(choice, torch.int32, "choice")
    if points2d.dim() != 4 or points2d.shape[0] != 7 or tuple(points2d.shape[2:]) != (38, 2):
        raise ValueError("points2d must be [7, T, 38, 2]")
    T = points2d.shape[1]
    if peak_pts.dim() != 5 or tuple(peak_pts.shape[:3]) != (7, T, 19) or peak_pts.shape[4] != 2 or tuple(choice.shape) != (7, T, 19):
        raise ValueError("peak_pts must be [7, T, 19, K, 2] and choice [7, T, 19] of the recording of points2d")
    if peak_pts.device != points2d.device or choice.device != points2d.device:
        raise ValueError("points2d, peak_pts and choice must be on one device")
    K = peak_pts.shape[3]
    slot = choice.to(torch.int64).clamp(0, K - 1)
    chosen = torch.gather(peak_pts, 3, slot[..., None, None].expand(7, T, 19, 1, 2)).squeeze(3).contiguous()
    # which of the 38 entries a moved chain fills: the re-layout leaves the row component as it is, and fills 0 where no chain does
    moved = (choice != 0).to(torch.float32)[..., None].expand(7, T, 19, 2).contiguous()
    replace = relayout_19_to_38(moved, camera_ordering)[..., 0] != 0.0
    return torch.where(replace[..., None], relayout_19_to_38(chosen, camera_ordering), points2d)


# ---- consensus triangulation over camera subsets ------------------------------------------------------------
@dataclasses.dataclass
class ConsensusResult:
    """What `triangulate_consensus` returns, device tensors but for the last: points3d [T, J, 3] float64, cameras [T, J] int32 (bit c set
    for each camera used), status [T, J] int8 (0 fewer than two views, 1 all views agree, 2 a proper subset was chosen, 3 no subset
    qualified: the all-views point), error [ncam, T, J] float64 (every view's reprojection error against the chosen point, rejected
    views included), fixed_px [ncam, T, J, 2] float64 (the detections with every rejected view replaced by the projection of the chosen
    point), counts [J, 4] int64 (how often each status occurred per joint) and params (tau [J], min_views)."""
    points3d: torch.Tensor
    cameras: torch.Tensor
    status: torch.Tensor
    error: torch.Tensor
    fixed_px: torch.Tensor
    counts: torch.Tensor
    params: tuple


def consensus_params(tau=None, min_views=None):
    """(tau, min_views) with config.ROBUST_TAU (20 px for each of the 38 joints, a guess nobody has measured on a recording) and
    config.ROBUST_MIN_VIEWS for what is None.  tau: one number for every joint, or one per joint; returned as a float64 array of one or
    J values.  ValueError: a tau that is no number, negative or NaN (+inf accepts every finite error), a min_views that is no integer
    in config.ROBUST_MIN_VIEWS_RANGE."""
    from . import config

    t = _per_joint(tau, config.ROBUST_TAU, "tau")
    return t, _integer(config.ROBUST_MIN_VIEWS if min_views is None else min_views, *config.ROBUST_MIN_VIEWS_RANGE, "min_views")


def _consensus_inputs(P, points2d_px, X):
    """(Ph, X, ncam, T, J): the checks the consensus and the trajectory entries share; X = triangulate() when None."""
    ncam, T, J = _need_points2d_px(points2d_px, bounded=True)
    Ph = _camera_matrices(P, ncam)
    if X is None:
        X = triangulate(Ph, points2d_px)
    else:
        _need_X(X, points2d_px)
    return Ph, X, ncam, T, J


@_on_tensor_device
def consensus_candidates(P, points2d_px, X=None):
    """Every candidate of the consensus triangulation at min_views = 2 (df3d_consensus_candidates), indexed by
    camera bitmask: (cand_X [T, J, 2^ncam, 3], cand_q [T, J, 2^ncam, ncam]) float64 on the device -- the DLT point of every subset of
    at least two views and the squared reprojection error of each of its cameras (+inf where the error is); 0 where a bitmask is no
    candidate.  Arguments as triangulate_consensus.  For tests: the production path never stores the candidates."""
    Ph, X, ncam, T, J = _consensus_inputs(P, points2d_px, X)
    dev = points2d_px.device
    cand_X = torch.zeros((T, J, 1 << ncam, 3), dtype=torch.float64, device=dev)
    cand_q = torch.zeros((T, J, 1 << ncam, ncam), dtype=torch.float64, device=dev)
    if T:
        _call("df3d_consensus_candidates", Ph.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), points2d_px.data_ptr(), X.data_ptr(), ncam, T, J,
              cand_X.data_ptr(), cand_q.data_ptr(), _stream(points2d_px))
    return cand_X, cand_q


@_on_tensor_device
def triangulate_consensus(P, points2d_px, X=None, tau=None, min_views=None):
    """The 3-D point of every (frame, joint) from the largest set of cameras that agree (df3d_triangulate_consensus, DESIGN.md section
    23), a ConsensusResult.  P [ncam, 3, 4] float64 (numpy or tensor, pixels); points2d_px [ncam, T, J, 2] float64 cuda (row_px, col_px);
    X [T, J, 3] float64 cuda = triangulate() of the same detections, computed when None.  Every subset of a joint's views with at least
    min_views cameras is triangulated; a subset qualifies when each of its cameras reprojects its point within tau[j] pixels; the
    largest qualifying subset wins, ties to the smaller sum of squared errors, then to the smaller bitmask.  Two views that agree with
    each other cannot be told from two correct ones: with three views and one wrong detection the wrong pair wins whenever the wrong
    detection lies near an epipolar line.  Defaults and refusals: consensus_params."""
    t, m = consensus_params(tau, min_views)   # refused before any device work
    Ph, X, ncam, T, J = _consensus_inputs(P, points2d_px, X)
    t = _broadcast_per_joint(t, J, "tau", "ROBUST_TAU" if tau is None else None)
    dev = points2d_px.device
    out = ConsensusResult(torch.empty((T, J, 3), dtype=torch.float64, device=dev), torch.empty((T, J), dtype=torch.int32, device=dev),
                          torch.empty((T, J), dtype=torch.int8, device=dev), torch.empty((ncam, T, J), dtype=torch.float64, device=dev),
                          torch.empty((ncam, T, J, 2), dtype=torch.float64, device=dev), torch.zeros((J, 4), dtype=torch.int64, device=dev), (t, m))
    if T:
        work, need = _workspace("df3d_consensus_work_bytes", ncam, T, J, device=dev, least=8)
        dp = ctypes.POINTER(ctypes.c_double)
        _call("df3d_triangulate_consensus", Ph.ctypes.data_as(dp), points2d_px.data_ptr(), X.data_ptr(), ncam, T, J, t.ctypes.data_as(dp), m,
              out.points3d.data_ptr(), out.cameras.data_ptr(), out.status.data_ptr(), out.error.data_ptr(), out.fixed_px.data_ptr(),
              out.counts.data_ptr(), work.data_ptr(), need, _stream(points2d_px))
    return out


# ---- trajectory triangulation: robust smoothing on the 2-D evidence ------------------------------------------
@dataclasses.dataclass
class TrajectoryResult:
    """What `triangulate_trajectory` returns, device tensors but for the last: points3d [T, J, 3] float64, status [T, J] int8 (0 not in
    a segment: the input's bits, 1 anchor, 2 filled frame with at least one view, 3 filled frame without a view, 4 a frame of a chain
    that did not converge: the last accepted iterate), weight [ncam, T, J] float64 (every view's final IRLS weight; below 1 names the
    camera to correct), error [ncam, T, J] float64 (every view's reprojection error against the final point), iterations [J] int32,
    cost [J, 2] float64 (start, final), counts [J, 5] int64 and params (lam [J], huber, max_gap, block_frames)."""
    points3d: torch.Tensor
    status: torch.Tensor
    weight: torch.Tensor
    error: torch.Tensor
    iterations: torch.Tensor
    cost: torch.Tensor
    counts: torch.Tensor
    params: tuple


def trajectory_params(lam=None, huber=None, max_gap=None, block_frames=None):
    """(lam, huber, max_gap, block_frames) with config.TRAJECTORY_LAMBDA (1e3 px^2 / mm^2 for each of the 38 joints),
    config.TRAJECTORY_HUBER (pixels) and config.REPAIR_MAX_GAP for what is None -- lam and huber are guesses nobody has measured on a
    recording; a block_frames of None stays None: the fit then takes config.trajectory_block_frames(T), which grows with sqrt(T).  lam: one number for every joint, or one per joint; returned as a float64 array of one
    or J values.  ValueError: a lam that is no number, negative or not finite, a huber that is no number, negative or NaN (+inf is plain
    least squares), a max_gap that is no integer in config.REPAIR_MAX_GAP_RANGE, a block_frames that is no integer in
    config.TRAJECTORY_BLOCK_FRAMES_RANGE."""
    from . import config

    l = _per_joint(lam, config.TRAJECTORY_LAMBDA, "lam", finite=True)
    h = _number(config.TRAJECTORY_HUBER if huber is None else huber, "huber")
    if not h >= 0.0:
        raise ValueError("huber must be >= 0 and not NaN (+inf is plain least squares)")
    gap = _integer(config.REPAIR_MAX_GAP if max_gap is None else max_gap, *config.REPAIR_MAX_GAP_RANGE, "max_gap")
    b = None if block_frames is None else _integer(block_frames, *config.TRAJECTORY_BLOCK_FRAMES_RANGE, "block_frames")
    return l, h, gap, b


def _trajectory_lambda(l, J, default):
    return _broadcast_per_joint(l, J, "lam", "TRAJECTORY_LAMBDA" if default else None)


def _trajectory_work(ncam, T, J, b, dev):
    """(work, bytes, block_frames): the workspace of the fit and the solve; block_frames None is config.trajectory_block_frames(T)."""
    from . import config

    b = config.trajectory_block_frames(T) if b is None else b
    refusal = f"no workspace for {{1}} frames: T must be at most {config.TRAJECTORY_MAX_FRAMES}"
    return (*_workspace("df3d_trajectory_work_bytes", ncam, T, J, b, device=dev, refusal=refusal), b)


@_on_tensor_device
def trajectory_linearize(P, points2d_px, X, huber=None):
    """(H [T, J, 6], g [T, J, 3], weight [ncam, T, J], error [ncam, T, J], cost [J]) float64 on the device: the Gauss-Newton terms of every
    frame's views at X [T, J, 3] (df3d_trajectory_linearize) and each chain's sum of Huber terms.  For tests."""
    h = trajectory_params(huber=huber)[1]
    Ph, X, ncam, T, J = _consensus_inputs(P, points2d_px, X)
    X, points2d_px = X.contiguous(), points2d_px.contiguous()
    dev = points2d_px.device
    out = (torch.zeros((T, J, 6), dtype=torch.float64, device=dev), torch.zeros((T, J, 3), dtype=torch.float64, device=dev),
           torch.zeros((ncam, T, J), dtype=torch.float64, device=dev), torch.zeros((ncam, T, J), dtype=torch.float64, device=dev),
           torch.zeros((J,), dtype=torch.float64, device=dev))
    if T:
        work = torch.empty((T * J,), dtype=torch.float64, device=dev)
        _call("df3d_trajectory_linearize", Ph.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), points2d_px.data_ptr(), X.data_ptr(), ncam, T, J,
              h, *(o.data_ptr() for o in out), work.data_ptr(), T * J * 8, _stream(points2d_px))
    return out


@_on_tensor_device
def trajectory_solve(H, g, segment, lam, mu, block_frames=None):
    """(d [T, J, 3] float64, ok [J] int32): one damped banded solve (H + lam K + mu I) d = -g of every chain (df3d_trajectory_solve, DESIGN.md
    section 24).  H [T, J, 6], g [T, J, 3] float64 cuda (the whole gradient), segment [T, J] int8 cuda (non-zero: the frame is an
    unknown).  For tests."""
    l, _, _, b = trajectory_params(lam=lam, block_frames=block_frames)
    _need(H, torch.float64, "H")
    _need(g, torch.float64, "g")
    _need(segment, torch.int8, "segment")
    if H.dim() != 3 or H.shape[2] != 6 or tuple(g.shape) != tuple(H.shape[:2]) + (3,) or tuple(segment.shape) != tuple(H.shape[:2]):
        raise ValueError("H must be [T, J, 6], g [T, J, 3] and segment [T, J]")
    T, J, _ = H.shape
    if not 1 <= J <= 64:
        raise ValueError("H must hold 1 to 64 joints")
    l = _trajectory_lambda(l, J, False)
    dev = H.device
    d = torch.zeros((T, J, 3), dtype=torch.float64, device=dev)
    ok = torch.ones((J,), dtype=torch.int32, device=dev)
    if T:
        work, need, b = _trajectory_work(1, T, J, b, dev)
        _call("df3d_trajectory_solve", H.contiguous().data_ptr(), g.contiguous().data_ptr(), segment.contiguous().data_ptr(), T, J,
              l.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(mu), b, d.data_ptr(), ok.data_ptr(), None, work.data_ptr(), need, _stream(H))
    return d, ok


@_on_tensor_device
def triangulate_trajectory(P, points2d_px, X=None, lam=None, huber=None, max_gap=None, block_frames=None):
    """The 3-D trajectory of every joint over the whole recording (df3d_triangulate_trajectory), a TrajectoryResult.
    P [ncam, 3, 4] float64 (numpy or tensor, pixels); points2d_px [ncam, T, J, 2] float64 cuda (row_px, col_px); X [T, J, 3] float64 cuda
    = triangulate() of the same detections, the start, computed when None.  Per joint the points minimise the Huber loss (huber, px) of
    every view's reprojection error plus lam (px^2 / mm^2) times the squared second differences of the trajectory, over every segment:
    a run of frames that starts and ends at a frame with two views and bridges at most max_gap frames without.  A frame one camera sees
    is fitted to that view and its neighbours; a frame outside every segment keeps its input.  The result does not depend on
    block_frames beyond rounding.  At most config.TRAJECTORY_MAX_FRAMES frames; a joint's whole iteration is one workgroup's work, about
    0.1 s per 1 000 frames of the slowest joint on an MI355X and not measured beyond 20 000 frames.  Defaults and refusals: trajectory_params."""
    l, h, gap, b = trajectory_params(lam, huber, max_gap, block_frames)   # refused before any device work
    Ph, X, ncam, T, J = _consensus_inputs(P, points2d_px, X)
    l = _trajectory_lambda(l, J, lam is None)
    dev = points2d_px.device
    out = TrajectoryResult(torch.empty((T, J, 3), dtype=torch.float64, device=dev), torch.empty((T, J), dtype=torch.int8, device=dev),
                           torch.empty((ncam, T, J), dtype=torch.float64, device=dev), torch.empty((ncam, T, J), dtype=torch.float64, device=dev),
                           torch.zeros((J,), dtype=torch.int32, device=dev), torch.zeros((J, 2), dtype=torch.float64, device=dev),
                           torch.zeros((J, 5), dtype=torch.int64, device=dev), (l, h, gap, b))
    if T:
        work, need, b = _trajectory_work(ncam, T, J, b, dev)
        out.params = (l, h, gap, b)
        dp = ctypes.POINTER(ctypes.c_double)
        _call("df3d_triangulate_trajectory", Ph.ctypes.data_as(dp), points2d_px.contiguous().data_ptr(), X.contiguous().data_ptr(), ncam, T, J,
              l.ctypes.data_as(dp), h, gap, b, out.points3d.data_ptr(), out.status.data_ptr(), out.weight.data_ptr(), out.error.data_ptr(),
              out.iterations.data_ptr(), out.cost.data_ptr(), out.counts.data_ptr(), work.data_ptr(), need, _stream(points2d_px))
    return out


def gaussian_window_taps(window_size, sigma, truncate=4.0):
    """[window_size] float64: what a Gaussian filter of deviation `sigma`, cut at int(truncate * sigma + 0.5) samples and applied
    to a line of `window_size` samples under nearest extension, multiplies each sample by to form output sample window_size // 2.
    Taps exp(-k^2 / 2 sigma^2) for |k| <= radius, normalised to sum 1; a tap that falls left of the line adds to sample 0, one
    that falls right of it to the last sample.  sigma = 0.1 has radius 0: the unit tap, the identity."""
    w, sigma = int(window_size), float(sigma)
    if w < 1 or not sigma > 0.0:
        raise ValueError("window_size must be >= 1 and sigma > 0")
    radius = int(float(truncate) * sigma + 0.5)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    taps = np.exp(-0.5 * (k / sigma) ** 2)
    taps /= taps.sum()
    folded = np.zeros(w, dtype=np.float64)
    np.add.at(folded, np.clip(w // 2 + np.arange(-radius, radius + 1), 0, w - 1), taps)
    return folded


SMOOTH_SIGMA, KEEP_SIGMA = 7.0, 0.1   # reference df3d/signal_util.py:151-154: a quiet window is smoothed, a lively one kept


@_on_tensor_device
def smooth_pose2d(points2d, window_size=20, std_thr=5.0):
    """Temporal smoothing of 2-D detections for display (reference df3d/signal_util.py:135-160),
    df3d_smooth_pose2d.  points2d [..., T, J, 2] float64 cuda with at most 8 leading cameras in all; every (camera, joint,
    coordinate) series is filtered along T: where the population deviation of the `window_size` samples around a frame is below
    `std_thr` the frame becomes their Gaussian (sigma 7) average, else it stays.  One launch; returns a new tensor of the same
    shape.  T = 0 returns an empty tensor.  The reference's `pad` argument only works at its default and is not exposed."""
    lib = _native.load()
    _need(points2d, torch.float64, "points2d")
    if points2d.dim() < 3 or points2d.shape[-1] != 2:
        raise ValueError("points2d must be [..., T, J, 2]")
    T, J = int(points2d.shape[-3]), int(points2d.shape[-2])
    C = int(np.prod(points2d.shape[:-3], dtype=np.int64))
    out = torch.empty_like(points2d)
    if C == 0 or J == 0:
        return out
    w = int(window_size)
    ws, wk = gaussian_window_taps(max(w, 1), SMOOTH_SIGMA), gaussian_window_taps(max(w, 1), KEEP_SIGMA)
    dp = ctypes.POINTER(ctypes.c_double)
    _native.check(
        lib.df3d_smooth_pose2d(points2d.data_ptr(), C, T, 2 * J, w, float(std_thr), ws.ctypes.data_as(dp), wk.ctypes.data_as(dp), out.data_ptr(),
                               _stream(points2d)),
        "df3d_smooth_pose2d",
    )
    return out


def filter_batch_2d(points2d, freq=100.0):
    """The reference's `filter_batch_2d` (df3d/signal_util.py:103-132) on the device: df3d_oneeuro_filter with its constants
    (mincutoff 1e-4, beta 30, dcutoff 1) and its time stamps, which start at 0 where `filter_batch`'s start at 0.1.
    points2d [T, J, 2] float64 cuda; bit-identical to the reference's float arithmetic."""
    return oneeuro_filter(points2d, freq=freq, mincutoff=1e-4, beta=30.0, dcutoff=1.0, first_stamp=0, stamp_step=0.1)


@_on_tensor_device
def render_heatmap(luma, heatmaps, planes, colors, flip, gain=1.0, cols=None, out=None):
    """Heat-maps drawn on camera images (df3d_render_heatmap), one launch for all views.
    luma [S, H, W] uint8 cuda and heatmaps [S, P, Hh, Wh] float32 cuda, one view per slot (1 <= S <= 8); `planes[s]` lists the planes of
    view s to draw (at most 32, any order), `colors[s]` one RGB triple per listed plane, `flip[s]` whether the network saw view s
    mirrored.  A single view may be given without the leading axis (luma [H, W], heatmaps [P, Hh, Wh], planes and colors of that view,
    flip a bool).  Every pixel shows (1 - a) grey + a colour of the plane whose bilinear sample, times `gain` and clamped to [0, 1], is
    the largest a there.  Returns [ceil(S / cols) H, cols W, 3] uint8 cuda, view s at grid cell (s // cols, s % cols); `cols` defaults
    to S (one row).  `out`: a contiguous uint8 CUDA tensor of at least that many bytes to draw into (bytes past the frame are not
    touched); cells of a last row that S does not fill are zero in a tensor made here and untouched in `out`."""
    lib = _native.load()
    if isinstance(luma, torch.Tensor) and luma.dim() == 2:
        luma, heatmaps, planes, colors, flip = luma.unsqueeze(0), heatmaps.unsqueeze(0), [planes], [colors], [flip]
    _need(luma, torch.uint8, "luma")
    _need(heatmaps, torch.float32, "heatmaps")
    if luma.dim() != 3 or heatmaps.dim() != 4 or heatmaps.shape[0] != luma.shape[0] or heatmaps.device != luma.device:
        raise ValueError("luma must be [S, H, W] and heatmaps [S, P, Hh, Wh] on one device")
    S, H, W = (int(v) for v in luma.shape)
    P, Hh, Wh = (int(v) for v in heatmaps.shape[1:])
    if not (len(planes) == len(colors) == len(flip) == S):
        raise ValueError("planes, colors and flip need one entry per view")
    cols = S if cols is None else int(cols)
    counts = [len(p) for p in planes]
    flat = np.asarray([int(q) for p in planes for q in p], dtype=np.int32)
    rgb = np.asarray([c for per_view in colors for c in per_view], dtype=np.int64).reshape(-1, 3)
    if len(rgb) != len(flat) or any(len(c) != n for c, n in zip(colors, counts)):
        raise ValueError("colors needs one RGB triple per selected plane")
    if rgb.size and (rgb.min() < 0 or rgb.max() > 255):
        raise ValueError("colors must lie in [0, 255]")
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    rows = -(-S // cols) if cols > 0 else 0
    need = rows * H * cols * W * 3
    if out is None:
        out = (torch.empty if rows * cols == S else torch.zeros)((rows * H, cols * W, 3), dtype=torch.uint8, device=luma.device)
    else:
        _need(out, torch.uint8, "out")
        if out.device != luma.device or out.numel() < need:
            raise ValueError(f"out must hold at least {need} bytes on the images' device")
    ip, up = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ubyte)
    _native.check(
        lib.df3d_render_heatmap(luma.data_ptr(), H, W, heatmaps.data_ptr(), P, Hh, Wh, S, cols, (ctypes.c_int * S)(*counts), flat.ctypes.data_as(ip),
                                rgb.ctypes.data_as(up), (ctypes.c_ubyte * S)(*[1 if f else 0 for f in flip]), float(gain), out.data_ptr(), _stream(luma)),
        "df3d_render_heatmap",
    )
    return out if tuple(out.shape) == (rows * H, cols * W, 3) else out.view(-1)[:need].view(rows * H, cols * W, 3)
