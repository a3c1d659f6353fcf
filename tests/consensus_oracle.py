"""Float64 numpy statement of the consensus triangulation of DESIGN.md section 23 (df3d_consensus_candidates,
df3d_triangulate_consensus).  TEST INFRASTRUCTURE ONLY.

Per point (t, j), detections (row_px, col_px), ncam <= 8:
    views       camera c is a view when both coordinates are non-zero; n = the number of views
    candidates  every subset S of the views with |S| >= max(min_views, 2); X_S = the DLT of the detections of S (here by SVD; the
                all-views candidate is `X_full`, given)
    error       [u, v, w] = P_c [X; 1] (reproj_oracle.project: left-to-right sums); du = u / w - col, dv = v / w - row,
                q = du du + dv dv, e = sqrt(q), +inf when w > 0 fails or e is not finite
    qualifies   every c in S has a finite e_c <= tau[j]
    choice      the largest |S|; then the smaller sse = sum of q_c over S in ascending camera order from 0.0; then the smaller bitmask
    status      0: n < 2 (X = 0, cameras = 0); 1: the all-views set was chosen (X = X_full); 2: a proper subset (X = X_S);
                3: none qualified (X = X_full, cameras = all views)
    err         [ncam, T, J]: every view's e against the chosen X (0 for non-views and at status 0)
    fixed_px    [ncam, T, J, 2]: the detections, every rejected view (a view outside the chosen set) replaced by (v / w, u / w)
    counts      [J, 4] int64
`choose` takes the candidate points as given (cand_X [T, J, 2^ncam, 3], indexed by camera bitmask), so that the kernel's choice is compared
on the kernel's own points; `candidates` computes them by SVD.
"""
import math

import numpy as np

from oracle import geometry as og
from reproj_oracle import project


def view_mask(px_point):
    """Bitmask of the views of one point, px_point [ncam, 2]."""
    return sum(1 << c for c in range(px_point.shape[0]) if px_point[c, 0] != 0.0 and px_point[c, 1] != 0.0)


def cams_of(mask):
    return [c for c in range(8) if mask >> c & 1]


def error(Pc, X, row, col):
    """(q, e, v / w, u / w) of one camera against one point.  Callers silence numpy's warnings (division by zero, NaN) once."""
    u, v, w = project(Pc, X)
    pu, pv = u / w, v / w
    du, dv = pu - col, pv - row
    q = du * du + dv * dv
    e = np.sqrt(q)
    if not (w > 0.0) or not math.isfinite(e):
        e = math.inf
    return q, e, pv, pu


def dlt(P, px):
    """oracle.geometry.triangulate_dlt_batched, [T, J, 3]; NaN where a view holds a NaN or an infinity (the SVD takes none)."""
    P, px = np.asarray(P, np.float64), np.asarray(px, np.float64)
    finite = np.isfinite(px).all(axis=-1)
    X = og.triangulate_dlt_batched(np.where(finite[..., None], px, 1.0), P)
    X[(og.visibility(px) & ~finite).any(axis=0)] = np.nan
    return X


def candidates(P, px):
    """cand_X [T, J, 2^ncam, 3] by SVD: the DLT of every subset of at least two views, 0 elsewhere (the all-views entry included)."""
    P, px = np.asarray(P, np.float64), np.asarray(px, np.float64)
    ncam, T, J, _ = px.shape
    vm = np.zeros((T, J), dtype=np.int64)
    for c in range(ncam):
        vm |= (og.visibility(px[c]).astype(np.int64)) << c
    out = np.zeros((T, J, 1 << ncam, 3))
    for mask in range(1 << ncam):
        cams = cams_of(mask)
        if len(cams) < 2:
            continue
        at = (vm & mask) == mask
        if not at.any():
            continue
        only = np.zeros_like(px)
        only[cams] = px[cams]
        out[:, :, mask][at] = dlt(P, only)[at]
    return out


def squared_errors(P, px, cand_X):
    """cand_q [T, J, 2^ncam, ncam]: q of every camera of every candidate against the candidate's point (+inf where e is); 0 elsewhere."""
    P, px = np.asarray(P, np.float64), np.asarray(px, np.float64)
    ncam, T, J, _ = px.shape
    out = np.zeros((T, J, 1 << ncam, ncam))
    old = np.seterr(all="ignore")
    for t in range(T):
        for j in range(J):
            vm = view_mask(px[:, t, j])
            for mask in range(1 << ncam):
                cams = cams_of(mask)
                if len(cams) < 2 or (vm & mask) != mask:
                    continue
                for c in cams:
                    q, e, _, _ = error(P[c], cand_X[t, j, mask], *px[c, t, j])
                    out[t, j, mask, c] = q if math.isfinite(e) else math.inf
    np.seterr(**old)
    return out


def key_of(P, px_point, X, mask, tau):
    """(qualifies, size, sse) of candidate `mask` with point X."""
    sse, ok = 0.0, True
    for c in cams_of(mask):
        q, e, _, _ = error(P[c], X, *px_point[c])
        sse = sse + q
        ok = ok and math.isfinite(e) and e <= tau
    return ok, len(cams_of(mask)), sse


def choose_point(P, px_point, cand_X_point, X_full, tau, min_views=2):
    """(X [3], cameras, status, err [ncam], fixed [ncam, 2]) of one point."""
    ncam = px_point.shape[0]
    vm = view_mask(px_point)
    n = len(cams_of(vm))
    err, fixed = np.zeros(ncam), np.array(px_point, dtype=np.float64)
    if n < 2:
        return np.zeros(3), 0, 0, err, fixed
    best = None
    for mask in range(1 << ncam):
        if (vm & mask) != mask or len(cams_of(mask)) < max(min_views, 2):
            continue
        X = X_full if mask == vm else cand_X_point[mask]
        ok, size, sse = key_of(P, px_point, X, mask, tau)
        if ok and (best is None or (-size, sse, mask) < best[0]):
            best = ((-size, sse, mask), X)
    if best is None:
        X, chosen, status = X_full, vm, 3
    else:
        X, chosen = best[1], best[0][2]
        status = 1 if chosen == vm else 2
    for c in cams_of(vm):
        _, e, pv, pu = error(P[c], X, *px_point[c])
        err[c] = e
        if not chosen >> c & 1:
            fixed[c] = (pv, pu)
    return np.array(X, dtype=np.float64), chosen, status, err, fixed


def choose(P, px, cand_X, X_full, tau, min_views=2):
    """(X [T, J, 3], cameras [T, J] int32, status [T, J] int8, err [ncam, T, J], fixed_px [ncam, T, J, 2], counts [J, 4] int64) on given
    candidate points.  tau: one value or [J]."""
    P, px = np.asarray(P, np.float64), np.asarray(px, np.float64)
    ncam, T, J, _ = px.shape
    tau = np.broadcast_to(np.asarray(tau, np.float64), (J,))
    X, cameras, status = np.zeros((T, J, 3)), np.zeros((T, J), np.int32), np.zeros((T, J), np.int8)
    err, fixed, counts = np.zeros((ncam, T, J)), np.zeros((ncam, T, J, 2)), np.zeros((J, 4), np.int64)
    old = np.seterr(all="ignore")
    for t in range(T):
        for j in range(J):
            X[t, j], cameras[t, j], status[t, j], err[:, t, j], fixed[:, t, j] = choose_point(P, px[:, t, j], cand_X[t, j], X_full[t, j], tau[j],
                                                                                                min_views)
            counts[j, status[t, j]] += 1
    np.seterr(**old)
    return X, cameras, status, err, fixed, counts


def consensus(P, px, tau, min_views=2):
    """The whole model on the oracle's own (SVD) points."""
    px = np.asarray(px, np.float64)
    return choose(P, px, candidates(P, px), dlt(P, px), tau, min_views)


def brute_force_choice(keys):
    """The winner of `keys` = [(mask, qualifies, size, sse)] by pairwise comparison alone: the candidate no other candidate beats.
    None when none qualifies."""
    def beats(a, b):
        if a[2] != b[2]:
            return a[2] > b[2]
        if a[3] != b[3]:
            return a[3] < b[3]
        return a[0] < b[0]

    live = [k for k in keys if k[1]]
    winners = [a for a in live if all(a is b or beats(a, b) for b in live)]
    assert len(winners) == (1 if live else 0)   # a total order has exactly one maximum
    return winners[0][0] if winners else None
