"""Float64 numpy restatement of the reprojection-error model of DESIGN.md section 10 (df3d_reproj_errors): plain loops over
(t, j, c), X taken as given.

    views       camera c sees (t, j) when both pixel coordinates are non-zero
    e[c, t, j]  0 unless (t, j) has >= 2 views and c is one of them; then [u, v, w] = P_c [X; 1] and
                e = sqrt((u / w - col)^2 + (v / w - row)^2), +inf when w <= 0 or e is not finite
    jmax[t, j]  max over c of e[c, t, j]
    mask[t]     bit j set when jmax[t, j] > thr[j]
"""
import math

import numpy as np


def project(P, X):
    """[u, v, w] of one 3x4 matrix and one point, each a left-to-right sum as the kernel writes it."""
    u = P[0, 0] * X[0] + P[0, 1] * X[1] + P[0, 2] * X[2] + P[0, 3]
    v = P[1, 0] * X[0] + P[1, 1] * X[1] + P[1, 2] * X[2] + P[1, 3]
    w = P[2, 0] * X[0] + P[2, 1] * X[1] + P[2, 2] * X[2] + P[2, 3]
    return u, v, w


def reproj_errors(P, pts_px, X, thr):
    """P [ncam, 3, 4], pts_px [ncam, T, J, 2] (row_px, col_px), X [T, J, 3], thr [J] -> (err [ncam, T, J], jmax [T, J], mask [T] int64)."""
    P = np.asarray(P, dtype=np.float64)
    pts_px = np.asarray(pts_px, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64)
    ncam, T, J, _ = pts_px.shape
    err = np.zeros((ncam, T, J))
    jmax = np.zeros((T, J))
    mask = np.zeros(T, dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(T):
            bits = 0
            for j in range(J):
                views = [c for c in range(ncam) if pts_px[c, t, j, 0] != 0.0 and pts_px[c, t, j, 1] != 0.0]
                if len(views) >= 2:
                    for c in views:
                        row, col = pts_px[c, t, j]
                        u, v, w = project(P[c], X[t, j])
                        du, dv = u / w - col, v / w - row
                        e = np.sqrt(du * du + dv * dv)
                        if not (w > 0.0) or not math.isfinite(e):
                            e = math.inf
                        err[c, t, j] = e
                jmax[t, j] = err[:, t, j].max() if ncam else 0.0
                if jmax[t, j] > thr[j]:
                    bits |= 1 << j
            mask[t] = np.array([bits], dtype=np.uint64).view(np.int64)[0]
    return err, jmax, mask


def flags(mask, J):
    """[T, J] bool table of the set bits of mask [T] int64."""
    m = np.asarray(mask, dtype=np.int64).view(np.uint64)
    return ((m[:, None] >> np.arange(J, dtype=np.uint64)) & np.uint64(1)).astype(bool)
