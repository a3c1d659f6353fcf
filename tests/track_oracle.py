"""The tracking model of DESIGN.md section 22 in numpy, float64 and int64: the definition that csrc/track.hip is compared with, exactly.

One chain is one (camera, network joint).  Inputs as ops.heatmap_peaks / Core.peaks lay them out: count [C, T, J] int32, pts [C, T, J,
K, 2] float32 (row / H, col / W), val [C, T, J, K] float32.

1. Slot k of frame t is valid when k < count and its value and both coordinates are finite.  A frame without a valid slot is a
   placeholder frame: slot 0 alone is valid, its unary cost is 0 and every pair cost to or from it is w_m.
2. u(t, k) = w_v min(v_best(t) - v(t, k), 1), v_best the largest valid value of the frame.
3. d(t; k', k) = w_m min(dr^2 + dc^2, tau^2) / tau^2, dr and dc the pixel differences (normalised x H, x W, in float64) between slot k of
   frame t and slot k' of frame t - 1.
4. Every u and d is computed in float64 in the order written and rounded once, q = rint(x 2^20) as int64; an invalid slot costs INF =
   2^61, and sums saturate at INF (INF + INF fits).  All costs are non-negative, so (min, +) with saturation is exactly associative.
5. Minimise sum_t q_u(t, k_t) + sum_{t >= 1} q_d(t; k_{t-1}, k_t).  The last frame takes the lowest slot among the minima and every
   back-pointer the lowest minimising predecessor: among the optimal paths, the one whose reversed sequence is lexicographically smallest.
6. choice [C, T, J] int32 (0 on placeholder frames), cost [C, J] int64.

`solve` is serial in time and vectorised over the chains; `brute_force` tries every path of a tiny case.
"""
import itertools

import numpy as np

INF = 1 << 61
SCALE = 2.0 ** 20
TAU, W_MOTION, W_VALUE, BLOCK_FRAMES = 30.0, 1.0, 1.0, 256   # config.TRACK_DEFAULTS
PAIR_CHUNK = 256   # frames whose pair tables are formed in one numpy statement


def quantise(x):
    return np.rint(np.asarray(x, dtype=np.float64) * SCALE).astype(np.int64)


def _chains(a):
    """[C, T, J, ...] -> [T, C J, ...]"""
    a = np.moveaxis(np.asarray(a), 1, 0)
    return a.reshape(a.shape[0], a.shape[1] * a.shape[2], *a.shape[3:])


def slots(count, pts, val, image_hw, w_value=W_VALUE):
    """(valid [T, N, K] bool, placeholder [T, N] bool, rows, cols [T, N, K] float64 pixels (0 where not a real peak), qu [T, N, K] int64)
    of the N = C J chains."""
    count, pts, val = _chains(count), _chains(pts), _chains(val)
    K = val.shape[-1]
    real = (np.arange(K) < count[..., None]) & np.isfinite(val) & np.isfinite(pts).all(axis=-1)
    placeholder = ~real.any(axis=-1)
    v = np.where(real, val, 0.0).astype(np.float64)
    best = np.where(real, v, -np.inf).max(axis=-1, initial=-np.inf)
    gap = np.where(real, np.where(placeholder, 0.0, best)[..., None] - v, 0.0)
    qu = np.where(real, quantise(w_value * np.minimum(gap, 1.0)), INF)
    valid = real.copy()
    valid[..., 0] |= placeholder
    qu[..., 0] = np.where(placeholder, 0, qu[..., 0])
    rows = np.where(real, pts[..., 0], 0.0).astype(np.float64) * float(image_hw[0])
    cols = np.where(real, pts[..., 1], 0.0).astype(np.float64) * float(image_hw[1])
    return valid, placeholder, rows, cols, qu


def pair_costs(valid, placeholder, rows, cols, t0, t1, tau=TAU, w_motion=W_MOTION):
    """qd [t1 - t0, N, K', K] int64 of the frames [t0, t1), t0 >= 1: from slot k' of frame t - 1 to slot k of frame t.  Entries of invalid
    slots are 0: their unary cost is INF already."""
    tt = float(tau) * float(tau)
    dr = rows[t0:t1, :, None, :] - rows[t0 - 1:t1 - 1, :, :, None]
    dc = cols[t0:t1, :, None, :] - cols[t0 - 1:t1 - 1, :, :, None]
    q = quantise(w_motion * np.minimum(dr * dr + dc * dc, tt) / tt)
    q = np.where((placeholder[t0:t1] | placeholder[t0 - 1:t1 - 1])[..., None, None], quantise(w_motion), q)
    return np.where(valid[t0:t1, :, None, :] & valid[t0 - 1:t1 - 1, :, :, None], q, 0)


def solve(count, pts, val, image_hw, tau=TAU, w_motion=W_MOTION, w_value=W_VALUE):
    """(choice [C, T, J] int32, cost [C, J] int64).  image_hw = (H, W) in pixels."""
    C, T, J = np.asarray(count).shape
    N = C * J
    if T == 0:
        return np.zeros((C, 0, J), np.int32), np.zeros((C, J), np.int64)
    valid, placeholder, rows, cols, qu = slots(count, pts, val, image_hw, w_value)
    K = qu.shape[-1]
    back = np.zeros((T, N, K), np.int8)
    a = qu[0].copy()
    lanes = np.arange(N)[:, None]
    for t0 in range(1, T, PAIR_CHUNK):
        t1 = min(T, t0 + PAIR_CHUNK)
        qd = pair_costs(valid, placeholder, rows, cols, t0, t1, tau, w_motion)
        for t in range(t0, t1):
            cand = np.minimum(a[:, :, None] + qd[t - t0], INF)          # [N, K', K]
            arg = cand.argmin(axis=1)                                     # the first minimum: the lowest predecessor
            back[t] = arg
            a = np.minimum(qu[t] + cand[lanes, arg, np.arange(K)], INF)
    k = a.argmin(axis=-1)
    cost = a.min(axis=-1)
    choice = np.zeros((T, N), np.int32)
    for t in range(T - 1, -1, -1):
        choice[t] = k
        k = back[t, np.arange(N), k]
    return np.ascontiguousarray(np.moveaxis(choice.reshape(T, C, J), 0, 1)), cost.reshape(C, J)


def brute_force(count, pts, val, image_hw, tau=TAU, w_motion=W_MOTION, w_value=W_VALUE):
    """solve's outputs by trying all K^T paths of every chain: the smallest saturated sum, and among the paths that reach it the one whose
    reversed sequence is lexicographically smallest."""
    C, T, J = np.asarray(count).shape
    valid, placeholder, rows, cols, qu = slots(count, pts, val, image_hw, w_value)
    K = qu.shape[-1]
    qd = pair_costs(valid, placeholder, rows, cols, 1, T, tau, w_motion) if T > 1 else None
    choice, cost = np.zeros((T, C * J), np.int32), np.zeros(C * J, np.int64)
    for n in range(C * J):
        best = None
        for reverse in itertools.product(range(K), repeat=T):   # in lexicographic order of the reversed path: the first minimum wins
            path = reverse[::-1]
            total = 0
            for t in range(T):
                total = min(total + int(qu[t, n, path[t]]), INF)
                if t:
                    total = min(total + int(qd[t - 1, n, path[t - 1], path[t]]), INF)
            if best is None or total < best[0]:
                best = (total, path)
        cost[n], choice[:, n] = best
    return np.ascontiguousarray(np.moveaxis(choice.reshape(T, C, J), 0, 1)), cost.reshape(C, J)
