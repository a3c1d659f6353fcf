"""Per-camera frame lags from epipolar consistency: which camera is how many frames late, from the detections and
the calibration alone, and the detections with the lags undone.  Host wrappers over csrc/sync.hip in the manner of ops.py (whose public
surface is pinned and stays as it is) with ops.py's one set of argument checks: device inputs and outputs are torch CUDA tensors, the
cost tables, the lag paths and the gather are libdf3d_hip.so kernels with no CPU fallback; the fundamental matrices and the cameras'
lags are small host computations in float64 and integers.  The model is stated in numpy / int64 by tests/sync_oracle.py.
"""
import ctypes
import dataclasses

import numpy as np
import torch

from . import config
from .ops import _call, _camera_matrices, _integer, _need, _need_points2d_px, _number, _on_tensor_device, _stream, _workspace

@dataclasses.dataclass
class SyncResult:
    """What `camera_sync` returns.  Host arrays: pairs [npair, 2] int32 (cameras a < b that share a joint), F [npair, 9] float64, lag
    [ncam, nW] int32 (camera c shows instant t in its frame t + lag[c, t // window]), status [ncam] int8 (0 unobservable: the camera
    shares no joint with another, 1 in step throughout, 2 lagging somewhere), pair_inconsistency [npair, nW] int32 (the pair's lag minus
    the difference of its cameras' lags: non-zero only where a triangle of pairs does not close) and params (max_lag, window, tau,
    switch, min_count).  Device tensors: pair_cost, pair_count [npair, nW, 2 max_lag + 1] int64 (the sum of the samples' costs in units
    of 2^-10 px^2 and their number, index lag + max_lag), pair_lag [npair, nW] int32, path_cost [npair] int64, pair_margin [npair, nW]
    float64 px^2 (the best other lag's mean cost minus the chosen one's; NaN below min_count samples) and points2d_px [ncam, T, J, 2]
    float64, the detections with every camera's lag undone (zeros where the frame does not exist)."""
    pairs: np.ndarray
    F: np.ndarray
    lag: np.ndarray
    status: np.ndarray
    pair_lag: torch.Tensor
    pair_margin: torch.Tensor
    pair_inconsistency: np.ndarray
    pair_cost: torch.Tensor
    pair_count: torch.Tensor
    path_cost: torch.Tensor
    points2d_px: torch.Tensor
    params: tuple


def sync_params(max_lag=None, window=None, tau=None, switch=None, min_count=None):
    """(max_lag, window, tau, switch, min_count) with config.SYNC_MAX_LAG, SYNC_WINDOW, SYNC_TAU, SYNC_SWITCH and SYNC_MIN_COUNT for what
    is None -- all guesses nobody has measured on a recording.  ValueError: a max_lag that is no integer in config.SYNC_MAX_LAG_RANGE, a
    window or min_count that is no integer >= 1, a tau that is no number in [0, config.SYNC_TAU_MAX], a switch that is no number in
    [0, config.SYNC_SWITCH_MAX]."""
    D = _integer(config.SYNC_MAX_LAG if max_lag is None else max_lag, *config.SYNC_MAX_LAG_RANGE, "max_lag")
    W = _integer(config.SYNC_WINDOW if window is None else window, 1, (1 << 31) - 1, "window")
    t = _number(config.SYNC_TAU if tau is None else tau, "tau")
    if not 0.0 <= t <= config.SYNC_TAU_MAX:
        raise ValueError(f"tau must be in [0, {config.SYNC_TAU_MAX:g}] and not NaN (it is {t!r})")
    k = _number(config.SYNC_SWITCH if switch is None else switch, "switch")
    if not 0.0 <= k <= config.SYNC_SWITCH_MAX:
        raise ValueError(f"switch must be in [0, {config.SYNC_SWITCH_MAX:g}] and not NaN (it is {k!r})")
    m = _integer(config.SYNC_MIN_COUNT if min_count is None else min_count, 1, (1 << 31) - 1, "min_count")
    return D, W, t, k, m


def _need_pairs(pairs, ncam):
    """pairs [npair, 2] as a contiguous int32 host array of cameras 0 <= a < b < ncam, no pair twice."""
    a = np.asarray(pairs)
    if a.size == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("pairs must be an integer array [npair, 2]")
    if not bool(np.all((0 <= a[:, 0]) & (a[:, 0] < a[:, 1]) & (a[:, 1] < ncam))) or len({(int(x), int(y)) for x, y in a}) != len(a):
        raise ValueError(f"pairs must hold distinct cameras 0 <= a < b < ncam ({ncam})")
    return np.ascontiguousarray(a, dtype=np.int32)


def fundamental_matrices(P, pairs):
    """F [npair, 9] float64 (row-major 3 x 3, unit Frobenius norm) of the camera pairs [npair, 2]: x_b^T F_ab x_a = 0 for the images
    x = (col_px, row_px, 1) of one 3-D point in cameras a and b.  From P [ncam, 3, 4] (numpy or tensor) on the host in float64 by the
    4 x 4 determinants of Hartley & Zisserman, eq. 17.3: F[j, i] = (-1)^(i + j) det [P_a without row i; P_b without row j].  No
    pseudo-inverse.  ValueError: two cameras with the same centre (F = 0: a norm below 1e-12 |P_a|^2 |P_b|^2, where cameras a baseline
    apart give 1e-4 and more)."""
    Ph = np.ascontiguousarray(P.detach().cpu().numpy() if isinstance(P, torch.Tensor) else P, dtype=np.float64)
    if Ph.ndim != 3 or Ph.shape[1:] != (3, 4):
        raise ValueError("P must be [ncam, 3, 4]")
    pairs = _need_pairs(pairs, Ph.shape[0])
    F = np.zeros((len(pairs), 3, 3), dtype=np.float64)
    for k, (a, b) in enumerate(pairs):
        for i in range(3):
            for j in range(3):
                M = np.concatenate([np.delete(Ph[a], i, axis=0), np.delete(Ph[b], j, axis=0)])
                F[k, j, i] = (-1.0) ** (i + j) * np.linalg.det(M)
        norm = np.sqrt(np.sum(F[k] * F[k]))
        if not (np.isfinite(norm) and norm > 1e-12 * np.sum(Ph[a] * Ph[a]) * np.sum(Ph[b] * Ph[b])):   # the determinants' rounding, not a matrix
            raise ValueError(f"cameras {a} and {b} have no fundamental matrix (the same centre, or a matrix that is not finite)")
        F[k] /= norm
    return F.reshape(-1, 9)


def sync_pairs(points2d_px, min_count=None):
    """pairs [npair, 2] int32, ascending: the cameras a < b that both detect some joint (no zero coordinate) in at least min_count frames.
    points2d_px [ncam, T, J, 2]: a tensor on any device, or a numpy array."""
    m = sync_params(min_count=min_count)[4]
    p = points2d_px if isinstance(points2d_px, torch.Tensor) else np.asarray(points2d_px)
    if p.ndim != 4 or p.shape[3] != 2:
        raise ValueError("points2d_px must be [ncam, T, J, 2]")
    if not (p.shape[1] and p.shape[2]):
        both = np.zeros((p.shape[0],) * 2)
    elif isinstance(p, torch.Tensor):
        seen = (p != 0).all(dim=3).to(torch.float64)                  # [ncam, T, J]
        both = torch.einsum("atj,btj->abj", seen, seen).max(dim=2).values.cpu().numpy()
    else:
        seen = (p != 0).all(axis=3).astype(np.float64)
        both = np.einsum("atj,btj->abj", seen, seen).max(axis=2)
    return np.array([(a, b) for a in range(p.shape[0]) for b in range(a + 1, p.shape[0]) if both[a, b] >= m], dtype=np.int32).reshape(-1, 2)


def _windows(T, W):
    return -(-T // W)


@_on_tensor_device
def sync_pair_costs(points2d_px, F, pairs, max_lag=None, window=None, tau=None):
    """(cost, count) [npair, nW, 2 max_lag + 1] int64 on the device (df3d_sync_pair_costs): per pair, window of
    camera a's frames and lag d, the sum of the samples' costs floor(min(e, tau^2) 2^10 + 0.5), e the squared Sampson distance of camera
    a's frame t and camera b's frame t + d against F, and the number of valid samples.  points2d_px [ncam, T, J, 2] float64 cuda
    (row_px, col_px), F [npair, 9] (fundamental_matrices), pairs [npair, 2]."""
    D, W, t, _, _ = sync_params(max_lag, window, tau)
    ncam, T, J = _need_points2d_px(points2d_px, bounded=True)
    pairs = _need_pairs(pairs, ncam)
    Fh = np.ascontiguousarray(F, dtype=np.float64)
    if Fh.shape != (len(pairs), 9):
        raise ValueError("F must be [npair, 9]")
    shape = (len(pairs), _windows(T, W), 2 * D + 1)
    cost = torch.zeros(shape, dtype=torch.int64, device=points2d_px.device)
    count = torch.zeros(shape, dtype=torch.int64, device=points2d_px.device)
    if len(pairs) and T:
        _call("df3d_sync_pair_costs", Fh.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
              len(pairs), points2d_px.data_ptr(), ncam, T, J, D, W, t, cost.data_ptr(), count.data_ptr(), _stream(points2d_px))
    return cost, count


@_on_tensor_device
def sync_paths(cost, count, switch=None, min_count=None):
    """(lag [npair, nW] int32, path_cost [npair] int64, margin [npair, nW] float64) on the device (df3d_sync_paths, DESIGN.md section
    28): per pair the lags that minimise the windows' costs plus floor(switch 2^10 + 0.5) per frame of lag changed between neighbouring
    windows -- an exact Viterbi on integers, ties to the smaller (|d|, d) --, that minimum, and per window the best other lag's mean
    cost minus the chosen one's in px^2 (NaN below min_count samples).  cost, count [npair, nW, 2 D + 1] int64 cuda."""
    _, _, _, k, m = sync_params(switch=switch, min_count=min_count)
    _need(cost, torch.int64, "cost")
    _need(count, torch.int64, "count")
    if cost.dim() != 3 or cost.shape != count.shape or cost.device != count.device or cost.shape[2] % 2 != 1:
        raise ValueError("cost and count must be [npair, nW, 2 D + 1] on one device")
    npair, nW, nL = cost.shape
    dev = cost.device
    lag = torch.zeros((npair, nW), dtype=torch.int32, device=dev)
    path_cost = torch.zeros((npair,), dtype=torch.int64, device=dev)
    margin = torch.full((npair, nW), float("nan"), dtype=torch.float64, device=dev)
    if npair and nW:
        work, need = _workspace("df3d_sync_work_bytes", npair, nW, nL // 2, device=dev,
                                refusal="no workspace for {0} pairs, {1} windows and max_lag {2}: at most 28 pairs, 1048576 windows, max_lag 64")
        _call("df3d_sync_paths", cost.data_ptr(), count.data_ptr(), npair, nW, nL // 2, int(np.floor(k * config.SYNC_COST_SCALE + 0.5)), m,
              lag.data_ptr(), path_cost.data_ptr(), margin.data_ptr(), work.data_ptr(), need, _stream(cost))
    return lag, path_cost, margin


def _lag_order(l):
    return (abs(int(l)), int(l))


def sync_camera_lags(pairs, pair_lag, count, ncam):
    """(lag [ncam, nW] int32, status [ncam] int8, inconsistency [npair, nW] int32) from the pairs' lags, on the host in integers (DESIGN.md
    section 28).  pairs [npair, 2]; pair_lag [npair, nW]; count [npair, nW, 2 D + 1] (sync_pair_costs').  Per window and connected
    component of the pair graph: the maximum spanning tree of the pairs, weighted by the count at the chosen lag, ties to the lower
    (a, b); the component's lowest camera at 0 and l_b = l_a + d_ab along the tree; then the component shifted so that its most frequent
    lag is 0, ties to the smaller (|l|, l).  status: 0 for a camera in a component of its own, 2 where some window's lag is not 0,
    else 1.  inconsistency = d_ab - (l_b - l_a)."""
    pairs = _need_pairs(pairs, ncam)
    d = np.asarray(pair_lag.cpu() if isinstance(pair_lag, torch.Tensor) else pair_lag).astype(np.int64)
    n = np.asarray(count.cpu() if isinstance(count, torch.Tensor) else count).astype(np.int64)
    if d.ndim != 2 or d.shape[0] != len(pairs) or n.ndim != 3 or n.shape[:2] != d.shape or n.shape[2] % 2 != 1:
        raise ValueError("pair_lag must be [npair, nW] and count [npair, nW, 2 D + 1]")
    D, nW = n.shape[2] // 2, d.shape[1]
    if d.size and np.abs(d).max() > D:
        raise ValueError(f"pair_lag must lie in [-{D}, {D}]")
    root = list(range(ncam))

    def find(c, r):
        while r[c] != c:
            c = r[c]
        return c

    for a, b in pairs:
        ra, rb = find(a, root), find(b, root)
        root[max(ra, rb)] = min(ra, rb)
    comp = [find(c, root) for c in range(ncam)]
    lag = np.zeros((ncam, nW), dtype=np.int64)
    for w in range(nW):
        weight = n[np.arange(len(pairs)), w, d[:, w] + D] if len(pairs) else np.zeros(0, dtype=np.int64)
        order = sorted(range(len(pairs)), key=lambda k: (-int(weight[k]), int(pairs[k, 0]), int(pairs[k, 1])))
        tree, links = list(range(ncam)), [[] for _ in range(ncam)]
        for k in order:
            a, b = int(pairs[k, 0]), int(pairs[k, 1])
            ra, rb = find(a, tree), find(b, tree)
            if ra != rb:
                tree[max(ra, rb)] = min(ra, rb)
                links[a].append((b, int(d[k, w])))
                links[b].append((a, -int(d[k, w])))
        for c0 in sorted(set(comp)):
            members, seen, todo = [c for c in range(ncam) if comp[c] == c0], {c0}, [c0]
            while todo:
                a = todo.pop()
                for b, step in links[a]:
                    if b not in seen:
                        seen.add(b)
                        lag[b, w] = lag[a, w] + step
                        todo.append(b)
            values = [int(lag[c, w]) for c in members]
            mode = min(set(values), key=lambda v: (-values.count(v), *_lag_order(v)))
            lag[members, w] -= mode
    status = np.array([0 if comp.count(comp[c]) == 1 else (2 if lag[c].any() else 1) for c in range(ncam)], dtype=np.int8)
    inc = (d - (lag[pairs[:, 1]] - lag[pairs[:, 0]])) if len(pairs) else np.zeros((0, nW), dtype=np.int64)
    return lag.astype(np.int32), status, inc.astype(np.int32)


@_on_tensor_device
def apply_sync(points2d_px, lag, window=None):
    """[ncam, T, J, 2] float64 on the device (df3d_sync_apply): camera c's detections of frame t + lag[c, t // window] at t, zeros where
    that frame does not exist.  points2d_px [ncam, T, J, 2] float64 cuda; lag [ncam, ceil(T / window)] integers (numpy or tensor)."""
    W = sync_params(window=window)[1]
    ncam, T, J = _need_points2d_px(points2d_px, bounded=True)
    l = np.asarray(lag.cpu() if isinstance(lag, torch.Tensor) else lag)
    if l.dtype.kind not in "iu" or l.shape != (ncam, _windows(T, W)) or (l.size and np.abs(l.astype(np.int64)).max() >= 1 << 31):
        raise ValueError(f"lag must be an integer array [ncam, nW] = [{ncam}, {_windows(T, W)}] of int32 values")
    out = torch.zeros_like(points2d_px)
    if T:
        ld = torch.from_numpy(np.ascontiguousarray(l, dtype=np.int32)).to(points2d_px.device)
        _call("df3d_sync_apply", points2d_px.data_ptr(), ld.data_ptr(), ncam, T, J, W, out.data_ptr(), _stream(points2d_px))
    return out


@_on_tensor_device
def camera_sync(P, points2d_px, max_lag=None, window=None, tau=None, switch=None, min_count=None):
    """The frame lag of every camera against the others of its group, from the epipolar consistency of the detections alone (DESIGN.md
    section 28), a SyncResult.  P [ncam, 3, 4] float64 (numpy or tensor, pixels); points2d_px [ncam, T, J, 2] float64 cuda (row_px,
    col_px).  Pairs of cameras that share a joint (sync_pairs), their fundamental matrices, the cost of every lag per window
    (sync_pair_costs), the pairs' lag paths (sync_paths), the cameras' lags (sync_camera_lags) and the detections with the lags undone
    (apply_sync).  Lags are relative within a connected group of pairs: with the fly layout a lag between the left and the right
    cameras cannot be seen, and in a group the majority is taken to be in step.  Defaults and refusals: sync_params."""
    D, W, t, k, m = sync_params(max_lag, window, tau, switch, min_count)   # refused before any device work
    ncam, T, J = _need_points2d_px(points2d_px, bounded=True)
    Ph = _camera_matrices(P, ncam)
    pairs = sync_pairs(points2d_px, m)
    F = fundamental_matrices(Ph, pairs)
    cost, count = sync_pair_costs(points2d_px, F, pairs, D, W, t)
    pair_lag, path_cost, margin = sync_paths(cost, count, k, m)
    lag, status, inc = sync_camera_lags(pairs, pair_lag, count, ncam)
    return SyncResult(pairs, F, lag, status, pair_lag, margin, inc, cost, count, path_cost, apply_sync(points2d_px, lag, W), (D, W, t, k, m))
