"""The camera-lag model of DESIGN.md section 28 in plain numpy and int64: every step of csrc/sync.hip and of sync.sync_camera_lags restated
with the same sample arithmetic in the same order and the same tie rules.  Every float64 product and sum below is one numpy operation
on arrays, so each is rounded on its own (no fused multiply-add), left to right as written.

    x = (col_px, row_px, 1);  l = F x_a;  m = F^T x_b;  s = x_b . l;  e = s s / (l0 l0 + l1 l1 + m0 m0 + m1 m1)
    q = floor(min(e, tau tau) 2^10 + 0.5) as int64 (a NaN costs tau tau); a sample with a zero denominator is skipped
"""
import numpy as np

SCALE = 1024.0


def windows(T, W):
    return -(-T // W)


def sample_costs(F, pa, pb, tau):
    """(q int64, valid bool) of the detections pa, pb [..., 2] (row_px, col_px) of cameras a and b against F [9]."""
    f = np.asarray(F, dtype=np.float64).reshape(9)
    ya, xa, yb, xb = pa[..., 0], pa[..., 1], pb[..., 0], pb[..., 1]
    valid = (xa != 0.0) & (ya != 0.0) & (xb != 0.0) & (yb != 0.0)
    with np.errstate(all="ignore"):
        l0 = f[0] * xa + f[1] * ya + f[2]
        l1 = f[3] * xa + f[4] * ya + f[5]
        l2 = f[6] * xa + f[7] * ya + f[8]
        m0 = f[0] * xb + f[3] * yb + f[6]
        m1 = f[1] * xb + f[4] * yb + f[7]
        s = xb * l0 + yb * l1 + l2
        den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1
        valid = valid & (den != 0.0)
        e = s * s / np.where(den != 0.0, den, 1.0)
        tau2 = np.float64(tau) * np.float64(tau)
        m = np.where(e < tau2, e, tau2)
        q = np.floor(m * SCALE + 0.5)
    return np.where(valid, q, 0.0).astype(np.int64), valid


def pair_costs(F, pairs, px, D, W, tau):
    """(cost, count) [npair, nW, 2 D + 1] int64 of px [C, T, J, 2]."""
    px = np.asarray(px, dtype=np.float64)
    T = px.shape[1]
    nW = windows(T, W)
    cost = np.zeros((len(pairs), nW, 2 * D + 1), dtype=np.int64)
    count = np.zeros_like(cost)
    win = np.arange(T) // W
    for k, (a, b) in enumerate(pairs):
        for d in range(-D, D + 1):
            t = np.arange(max(0, -d), min(T, T - d))   # camera a's frames whose partner t + d exists
            if t.size == 0:
                continue
            q, valid = sample_costs(F[k], px[a][t], px[b][t + d], tau)
            np.add.at(cost[k, :, d + D], win[t], q.sum(axis=1))
            np.add.at(count[k, :, d + D], win[t], valid.sum(axis=1).astype(np.int64))
    return cost, count


def lag_order(d):
    return (abs(int(d)), int(d))


def paths(cost, count, kq, min_count):
    """(lag [npair, nW] int32, path_cost [npair] int64, margin [npair, nW] float64): the exact Viterbi in Python integers."""
    npair, nW, nL = cost.shape
    D = nL // 2
    ranked = sorted(range(-D, D + 1), key=lag_order)
    lag = np.zeros((npair, nW), dtype=np.int32)
    total = np.zeros(npair, dtype=np.int64)
    margin = np.full((npair, nW), np.nan)
    for k in range(npair):
        if nW == 0:
            continue
        V = [int(v) for v in cost[k, 0]]
        back = []
        for w in range(1, nW):
            new, frm = [], []
            for s in range(nL):
                best = None
                for d in ranked:
                    v = V[d + D] + int(kq) * abs(d + D - s)
                    if best is None or v < best:
                        best, at = v, d + D
                new.append(int(cost[k, w, s]) + best)
                frm.append(at)
            V = new
            back.append(frm)
        best = None
        for d in ranked:
            if best is None or V[d + D] < best:
                best, s = V[d + D], d + D
        total[k] = best
        for w in range(nW - 1, -1, -1):
            lag[k, w] = s - D
            if w > 0:
                s = back[w - 1][s]
        for w in range(nW):
            s = int(lag[k, w]) + D
            n = count[k, w]
            if n[s] >= min_count and n[s] > 0:
                here = np.float64(cost[k, w, s]) / np.float64(n[s]) / SCALE
                other = [np.float64(cost[k, w, j]) / np.float64(n[j]) / SCALE for j in range(nL) if j != s and n[j] > 0]
                margin[k, w] = (min(other) if other else np.inf) - here
    return lag, total, margin


def camera_lags(pairs, pair_lag, count, ncam):
    """(lag [ncam, nW] int32, status [ncam] int8, inconsistency [npair, nW] int32)."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    npair, nW = len(pairs), np.asarray(pair_lag).shape[1]
    D = np.asarray(count).shape[2] // 2
    comp = list(range(ncam))   # the lowest camera of each camera's connected component
    changed = True
    while changed:
        changed = False
        for a, b in pairs:
            lo = min(comp[a], comp[b])
            if comp[a] != lo or comp[b] != lo:
                comp[a] = comp[b] = lo
                changed = True
    lag = np.zeros((ncam, nW), dtype=np.int64)
    inc = np.zeros((npair, nW), dtype=np.int64)
    for w in range(nW):
        d = [int(pair_lag[k][w]) for k in range(npair)]
        weight = [int(count[k][w][d[k] + D]) for k in range(npair)]
        group = list(range(ncam))   # Kruskal's forest
        tree = []
        for k in sorted(range(npair), key=lambda k: (-weight[k], pairs[k])):
            a, b = pairs[k]
            if group[a] != group[b]:
                tree.append(k)
                old, new = group[b], group[a]
                group = [new if g == old else g for g in group]
        for root in sorted(set(comp)):
            members = [c for c in range(ncam) if comp[c] == root]
            known = {root: 0}
            while len(known) < len(members):
                for k in tree:
                    a, b = pairs[k]
                    if a in known and b not in known:
                        known[b] = known[a] + d[k]
                    elif b in known and a not in known:
                        known[a] = known[b] - d[k]
            values = [known[c] for c in members]
            mode = sorted(set(values), key=lambda v: (-values.count(v), abs(v), v))[0]
            for c in members:
                lag[c, w] = known[c] - mode
        for k, (a, b) in enumerate(pairs):
            inc[k, w] = d[k] - (lag[b, w] - lag[a, w])
    status = np.zeros(ncam, dtype=np.int8)
    for c in range(ncam):
        if comp.count(comp[c]) > 1:
            status[c] = 2 if np.any(lag[c] != 0) else 1
    return lag.astype(np.int32), status, inc.astype(np.int32)


def apply(px, lag, W):
    """Camera c's frame t + lag[c, t // W] at t, zeros where that frame does not exist."""
    px = np.asarray(px)
    C, T = px.shape[:2]
    out = np.zeros_like(px)
    for c in range(C):
        for t in range(T):
            src = t + int(lag[c][t // W])
            if 0 <= src < T:
                out[c, t] = px[c, src]
    return out


def find_pairs(px, min_count):
    px = np.asarray(px)
    seen = (px != 0).all(axis=3)
    C = px.shape[0]
    return [(a, b) for a in range(C) for b in range(a + 1, C) if px.shape[1] and px.shape[2] and (seen[a] & seen[b]).sum(axis=0).max() >= min_count]
