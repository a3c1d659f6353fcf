"""Float64 numpy restatement of the temporal smoothing of 2-D detections: the semantics of the reference's
`smooth_pose2d` (df3d/signal_util.py:135-160) in collapsed form.  The kernel df3d_smooth_pose2d is tested against this file, and this
file against outputs of the reference itself (tests/golden/smooth_golden.npz, tests/test_smooth_host.py).

The reference filters each 20-sample window with scipy's gaussian_filter1d(mode="nearest") and keeps output sample 10.  The Gaussian
is cut at int(4 sigma + 0.5) samples: 28 for sigma = 7, so most of its 57 taps fall outside the 20-sample line and multiply the line's
first or last sample.  The result is a fixed weighted sum of the 20 samples (`window_taps`); sigma = 0.1 has radius 0, the identity.
"""
import numpy as np


def window_taps(window_size, sigma, truncate=4.0):
    """[window_size] coefficients of output sample window_size // 2 (written independently of ops.gaussian_window_taps: a loop)."""
    radius = int(truncate * sigma + 0.5)
    g = [np.exp(-0.5 * (k / sigma) ** 2) for k in range(-radius, radius + 1)]
    total = float(np.sum(g))
    folded = np.zeros(window_size, dtype=np.float64)
    for k in range(-radius, radius + 1):
        folded[min(max(window_size // 2 + k, 0), window_size - 1)] += g[k + radius] / total
    return folded


def windows(points, window_size):
    """[..., T, nch] -> [..., T, nch, window_size]: samples t - W/2 .. t + W/2 - 1 of the edge-replicated series."""
    x = np.asarray(points, dtype=np.float64)
    T, half = x.shape[-2], window_size // 2
    idx = np.clip(np.arange(T)[:, None] + np.arange(-half, window_size - half)[None, :], 0, max(T - 1, 0))   # [T, W]
    return np.moveaxis(x[..., idx, :], -2, -1) if T else np.zeros(x.shape + (window_size,))


def window_std(points, window_size=20):
    """Population deviation of every window, [..., T, nch] (NaN where a window holds a NaN or an infinity)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.std(windows(points, window_size), axis=-1)


def smooth(points, window_size=20, std_thr=5.0, w_smooth=None, w_keep=None):
    """[..., T, nch] -> (out, std): sum_k w_smooth[k] x[k] where std < std_thr, else sum over the non-zero taps of w_keep."""
    w_smooth = window_taps(window_size, 7.0) if w_smooth is None else np.asarray(w_smooth, dtype=np.float64)
    w_keep = window_taps(window_size, 0.1) if w_keep is None else np.asarray(w_keep, dtype=np.float64)
    win = windows(points, window_size)
    with np.errstate(invalid="ignore", over="ignore"):
        std = np.std(win, axis=-1)
        smoothed = win @ w_smooth
        live = np.nonzero(w_keep)[0]
        kept = win[..., live] @ w_keep[live]
    return np.where(std < std_thr, smoothed, kept), std


def smooth_pose2d(points2d, window_size=20, std_thr=5.0):
    """[..., T, J, 2] -> the same shape, as ops.smooth_pose2d."""
    p = np.asarray(points2d, dtype=np.float64)
    flat = p.reshape(p.shape[:-2] + (p.shape[-2] * 2,))
    return smooth(flat, window_size, std_thr)[0].reshape(p.shape)
