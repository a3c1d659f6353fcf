"""Float64 numpy restatement of the pictorial-structures correction.  This module DEFINES the model the
device kernels (deepfly3d_amd/csrc/pictorial.hip) implement; it is not a port of DeepFly3D 0.x's solver, which the reference
checkout does not contain.  Test infrastructure only (not collected: no test_ prefix); numpy, plus the existing numpy oracle of
the 19 -> 38 re-layout (oracle/geometry.py).
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import geometry as og  # noqa: E402

NJ, NPRED = 38, 19


# ---------------------------------------------------------------------------------------------------------------- 1. peaks
def heatmap_peaks(hm, k):
    """hm [n, J, H, W] float32 -> count [n, J] int32, points [n, J, k, 2] float32 (row/H, col/W), values [n, J, k] float32.
    A cell is a peak when it is finite, > every finite 8-neighbour before it in row-major order and >= every finite one after
    it; the k best by value descending, then flat index ascending; unused slots zero."""
    hm = np.asarray(hm, np.float32)
    n, J, H, W = hm.shape
    pad = np.full((n, J, H + 2, W + 2), np.nan, np.float32)
    pad[:, :, 1:-1, 1:-1] = hm
    fin = np.isfinite(hm)
    peak = fin.copy()
    with np.errstate(invalid="ignore"):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr == 0 and dc == 0:
                    continue
                q = pad[:, :, 1 + dr : 1 + dr + H, 1 + dc : 1 + dc + W]
                before = dr < 0 or (dr == 0 and dc < 0)
                ok = (hm > q) if before else (hm >= q)
                peak &= ok | ~np.isfinite(q)
    count = np.zeros((n, J), np.int32)
    pts = np.zeros((n, J, k, 2), np.float32)
    vals = np.zeros((n, J, k), np.float32)
    inv_h, inv_w = np.float32(1) / np.float32(H), np.float32(1) / np.float32(W)
    flat, pflat = hm.reshape(n, J, H * W), peak.reshape(n, J, H * W)
    for a in range(n):
        for b in range(J):
            idx = np.flatnonzero(pflat[a, b])
            v = flat[a, b, idx]
            sel = idx[np.lexsort((idx, -v))][:k]
            count[a, b] = sel.size
            pts[a, b, : sel.size, 0] = (sel // W).astype(np.float32) * inv_h
            pts[a, b, : sel.size, 1] = (sel % W).astype(np.float32) * inv_w
            vals[a, b, : sel.size] = flat[a, b, sel]
    return count, pts, vals


# ---------------------------------------------------------------------------------------------------------------- cameras
def seeing_table(camera_ordering):
    """For every output joint j: [(camera, network joint, left), ...] of the cameras that see it, in increasing camera index --
    read off the re-layout's own rule (oracle/geometry.py:relayout_19_to_38 applied to marker inputs), not a second table."""
    marks = np.zeros((7, 1, NPRED, 2))
    marks[:, 0, :, 0] = np.arange(1, NPRED + 1)
    marks[:, 0, :, 1] = 0.25
    out = og.relayout_19_to_38(marks, list(camera_ordering))[:, 0]   # row = network joint + 1 where seen; col 0.75 on left cameras
    return [[(c, int(out[c, j, 0]) - 1, bool(out[c, j, 1] == 0.75)) for c in range(7) if out[c, j, 0] > 0] for j in range(NJ)]


def _dlt(rows_px, P):
    """rows_px: list of (cam, row_px, col_px); the DLT of the views with both coordinates != 0 (>= 2 needed, else 0)."""
    A = []
    for c, row, col in rows_px:
        if row != 0.0 and col != 0.0:
            A.append(col * P[c, 2] - P[c, 0])
            A.append(row * P[c, 2] - P[c, 1])
    if len(A) < 4:
        return np.zeros(3)
    X = np.linalg.svd(np.asarray(A))[2][-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return X[:3] / X[3]


# ---------------------------------------------------------------------------------------------------------------- 2-3. proposals
def proposals(P, camera_ordering, argmax2d, count, pts, vals, image_shape, k, m, tau=30.0, w_r=1.0, w_h=1.0, joints=None):
    """All proposals and the kept set of every (frame, joint).  argmax2d [7, T, 38, 2] normalised (the re-layout of the arg-max
    detections); count / pts / vals [7, T, 19, ...] the peaks of the network's planes; image_shape [W, H].
    Returns {"all": [T][38] dict(index, X, U, match), "kept": [T][38] dict(index, X, U, match)} (numpy arrays); with `joints`
    only those joints are computed (None in the other places)."""
    P = np.asarray(P, np.float64)
    W, H = float(image_shape[0]), float(image_shape[1])
    table = seeing_table(camera_ordering)
    T = argmax2d.shape[1]
    res_all, res_kept = [], []
    for t in range(T):
        row_all, row_kept = [], []
        for j in range(NJ):
            if joints is not None and j not in joints:
                row_all.append(None)
                row_kept.append(None)
                continue
            see = table[j]
            ns = len(see)
            cnt = [int(min(max(count[c, t, s], 0), k)) for c, s, _ in see]
            prow, pcol, pval = [], [], []
            for (c, s, left), n in zip(see, cnt):
                r = pts[c, t, s, :n, 0].astype(np.float64)
                cl = pts[c, t, s, :n, 1].astype(np.float64)
                if left:
                    cl = 1.0 - cl
                prow.append(r * H)
                pcol.append(cl * W)
                pval.append(vals[c, t, s, :n].astype(np.float64))
            idx, Xs = [0], [_dlt([(c, argmax2d[c, t, j, 0] * H, argmax2d[c, t, j, 1] * W) for c in range(7)], P)]
            pairs = [(0, 1), (0, 2), (1, 2)][: ns * (ns - 1) // 2]
            for q, (a, b) in enumerate(pairs):
                for i in range(cnt[a]):
                    for jj in range(cnt[b]):
                        idx.append(1 + q * k * k + i * k + jj)
                        Xs.append(_dlt([(see[a][0], prow[a][i], pcol[a][i]), (see[b][0], prow[b][jj], pcol[b][jj])], P))
            idx, X = np.asarray(idx), np.asarray(Xs)
            U = np.zeros(len(idx))
            match = np.zeros(len(idx), np.int64)
            finite = np.isfinite(X).all(axis=1)
            for a, (c, _, _) in enumerate(see):
                with np.errstate(invalid="ignore", over="ignore"):
                    u = X @ P[c, :, :3].T + P[c, :, 3]
                d = np.full(len(idx), float(tau))
                h = np.zeros(len(idx))
                best = np.zeros(len(idx), np.int64)
                ok = finite & (u[:, 2] > 0) & (cnt[a] > 0)
                if ok.any():
                    x, y = u[ok, 0] / u[ok, 2], u[ok, 1] / u[ok, 2]
                    d2 = (x[:, None] - pcol[a][None, :]) ** 2 + (y[:, None] - prow[a][None, :]) ** 2
                    d2 = np.where(np.isnan(d2), np.inf, d2)
                    b = np.argmin(d2, axis=1)
                    dmin = d2[np.arange(len(b)), b]
                    hit = np.isfinite(dmin)
                    sel = np.flatnonzero(ok)
                    d[sel[hit]] = np.sqrt(dmin[hit])
                    h[sel[hit]] = pval[a][b[hit]]
                    best[sel[hit]] = b[hit]
                dd = np.minimum(d, tau)
                U = U + (w_r * (dd * dd) / (tau * tau) - w_h * h)
                match |= best << (8 * a)
            U = np.where(np.isnan(U), np.inf, U)
            others = np.lexsort((idx[1:], U[1:]))[: m - 1] + 1
            keep = np.concatenate([[0], others]).astype(np.int64)
            row_all.append({"index": idx, "X": X, "U": U, "match": match})
            row_kept.append({"index": idx[keep], "X": X[keep], "U": U[keep], "match": match[keep]})
        res_all.append(row_all)
        res_kept.append(row_kept)
    return {"all": res_all, "kept": res_kept}


# ---------------------------------------------------------------------------------------------------------------- 4-5. solve
def chains_from_parent(parent):
    """Chains of a parent table (every joint parents at most one joint), root first, roots in increasing joint order."""
    parent = list(parent)
    child = {p: j for j, p in enumerate(parent) if p >= 0}
    assert len(child) == sum(p >= 0 for p in parent), "a joint parents two joints: not a set of chains"
    out = []
    for r, p in enumerate(parent):
        if p < 0:
            ch = [r]
            while ch[-1] in child:
                ch.append(child[ch[-1]])
            out.append(ch)
    return out


def _bone(Xp, Xc, mu, sigma, w_b):
    """[np, nc] bone costs w_b ((|X_parent - X_child| - mu) / sigma)^2."""
    diff = Xp[:, None, :] - Xc[None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (np.sqrt((diff * diff).sum(-1)) - mu) * (1.0 / sigma)
        return w_b * (z * z)


def chain_dp(U, X, mu, sigma, w_b=1.0):
    """Exact min-sum along one chain (root first): U[e] [n_e] unary costs, X[e] [n_e, 3] proposals, mu / sigma[e] of the bone
    (e - 1, e).  Leaves to root, ties to the lowest index, NaN as +inf.  Returns (energy, [choice per joint])."""
    L = len(U)
    cost = np.asarray(U[-1], np.float64)
    args = [None] * L
    for e in range(L - 1, 0, -1):
        v = cost[None, :] + _bone(np.asarray(X[e - 1]), np.asarray(X[e]), mu[e], sigma[e], w_b)
        v = np.where(np.isnan(v), np.inf, v)
        a = np.argmin(v, axis=1)
        args[e] = a
        cost = np.asarray(U[e - 1], np.float64) + v[np.arange(len(a)), a]
    cost = np.where(np.isnan(cost), np.inf, cost)
    ch = [int(np.argmin(cost))]
    energy = float(cost[ch[0]])
    for e in range(1, L):
        ch.append(int(args[e][ch[-1]]))
    return energy, ch


def chain_energy(U, X, mu, sigma, choice, w_b=1.0):
    e = sum(float(U[i][choice[i]]) for i in range(len(U)))
    for i in range(1, len(U)):
        e += float(_bone(np.asarray(X[i - 1])[choice[i - 1]][None], np.asarray(X[i])[choice[i]][None], mu[i], sigma[i], w_b)[0, 0])
    return e


def chain_brute(U, X, mu, sigma, w_b=1.0):
    """Enumerate every assignment of one chain: (energy, choice) of the minimum (lexicographically first on ties)."""
    import itertools

    best, arg = np.inf, None
    for choice in itertools.product(*[range(len(u)) for u in U]):
        e = chain_energy(U, X, mu, sigma, choice, w_b)
        if e < best:
            best, arg = e, list(choice)
    return best, arg


def solve(kept, camera_ordering, argmax2d, count, pts, parent, bone, w_b=1.0, k=None):
    """The exact solve of every frame on the kept proposals.  Returns (points2d [7, T, 38, 2], choice [T, 38] proposal index,
    energy [T], margin [T, 38] = the gap of each chain's best energy to the best with another choice at that joint
    (inf when there is none))."""
    T = argmax2d.shape[1]
    table = seeing_table(camera_ordering)
    out = np.array(argmax2d, np.float64, copy=True)
    choice = np.zeros((T, NJ), np.int64)
    energy = np.zeros(T)
    margin = np.full((T, NJ), np.inf)
    k = pts.shape[3] if k is None else k
    chains = chains_from_parent(parent)
    for t in range(T):
        e_t = 0.0
        for ch in chains:
            U = [kept[t][j]["U"] for j in ch]
            X = [kept[t][j]["X"] for j in ch]
            mu = [bone[j][0] for j in ch]
            sg = [bone[j][1] if parent[j] >= 0 else 1.0 for j in ch]
            e, sel = chain_dp(U, X, mu, sg, w_b)
            e_t += e
            for pos_in_chain, j in enumerate(ch):
                # runner-up with another proposal at this joint: the DP with the chosen one forbidden
                if len(U[pos_in_chain]) > 1:
                    U2 = [u.copy() for u in U]
                    U2[pos_in_chain][sel[pos_in_chain]] = np.inf
                    margin[t, j] = chain_dp(U2, X, mu, sg, w_b)[0] - e
                s = sel[pos_in_chain]
                choice[t, j] = kept[t][j]["index"][s]
                mword = int(kept[t][j]["match"][s])
                for a, (c, src, left) in enumerate(table[j]):
                    n = int(min(max(count[c, t, src], 0), k))
                    if n > 0:
                        sl = min((mword >> (8 * a)) & 0xFF, n - 1)
                        r, cl = float(pts[c, t, src, sl, 0]), float(pts[c, t, src, sl, 1])
                        out[c, t, j] = (r, 1.0 - cl if left else cl)
        energy[t] = e_t
    return out, choice, energy, margin
