"""The model of the heat-map triangulation in float64 numpy: the specification csrc/heatmap3d.hip is compared with.

For a candidate 3-D point, every camera that has a heat-map plane for the joint is asked what its heat-map says at the point's
projection; the point is where the sum of the logarithms (the product of the heat-maps) is largest.  Every operation below is one
float64 operation of the kernel, in the kernel's order (the file is built with -ffp-contract=off):

  cell value   l = log(h) where h > floor and h is finite, else log_floor = log(floor): NaN, +-inf and negatives go to the floor.
               (The kernel never sees `floor`: it compares log(h) > log_floor, the same decision for every float32 h != floor, because
               two different float32 values lie 6e-8 apart relatively and their logarithms 6e-8 absolutely.  Where `floor` is itself a
               float32 and h equals it, the decision rests on the device's logarithm and numpy's giving the same double for that
               one value: tests/heatmap3d_cases.py's "floor" case runs it at 2^-10, and they do.)
  projection   u = P00 x + P01 y + P02 z + P03 (left to right), v and w alike; col_px = u / w, row_px = v / w
  cells        r = row_px / cell_rows, c = col_px / cell_cols, for a flipped view c = W - col_px / cell_cols
  weights      Catmull-Rom at f = r - floor(r):  ((-f + 2) f - 1) f / 2,  ((3 f - 5) f f + 2) / 2,  ((-3 f + 4) f + 1) f / 2,
               (f - 1) f f / 2, every product left to right
  sample       taps floor(r) - 1 .. floor(r) + 2 by floor(c) - 1 .. floor(c) + 2, indices clamped to the plane; the four columns of a
               row are summed in ascending order starting from the first product, then the four rows alike
               a sample none of whose 16 taps lies above log_floor is log_floor itself: the weights do not add up to 1 to the last bit,
               and "no evidence in reach" must not depend on that
  view         max(sample, log_floor) when w > 0 and 0 <= r <= H - 1 and 0 <= c <= W - 1, else log_floor
  score        0.0 + view + view + ... over the joint's views in ascending order
  search       G = 8: level l scores the 512 points centre + (i - 3.5) step per axis, step = 2 half_l / 8, index (ix 8 + iy) 8 + iz; the
               best is the largest score, ties to the lowest index; the next level has centre = that point and half = step
  status       0 fewer than two views, X0 not finite or X0 = (0, 0, 0): the bits of X0, score NaN, shift 0, choice -1
               2 no point of level 0 scored above the all-floor score (log_floor added up once per view): X0, that score, choice -1
               3 searched, and the best point of level 0 lay on a face of the cube;  1 searched
"""
import numpy as np

GRID = 8
_OFF = np.arange(GRID, dtype=np.float64) - 3.5


def cell_logs(plane, floor, log_floor):
    """l [H, W] float64 of one float32 plane."""
    h = np.asarray(plane, dtype=np.float32).astype(np.float64)
    ok = np.isfinite(h) & (h > floor)
    with np.errstate(all="ignore"):
        return np.where(ok, np.log(np.where(ok, h, 1.0)), log_floor)


def project(P, X):
    """(row_px, col_px, w) of points X [..., 3] under one camera P [3, 4]."""
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        u = P[0, 0] * x + P[0, 1] * y + P[0, 2] * z + P[0, 3]
        v = P[1, 0] * x + P[1, 1] * y + P[1, 2] * z + P[1, 3]
        w = P[2, 0] * x + P[2, 1] * y + P[2, 2] * z + P[2, 3]
        return v / w, u / w, w


def to_cells(row_px, col_px, flip, cell, W):
    with np.errstate(all="ignore"):
        r = row_px / cell[0]
        c = col_px / cell[1]
        return r, (W - c if flip else c)


def weights(f):
    return (((-f + 2.0) * f - 1.0) * f * 0.5, ((3.0 * f - 5.0) * f * f + 2.0) * 0.5, ((-3.0 * f + 4.0) * f + 1.0) * f * 0.5,
            (f - 1.0) * f * f * 0.5)


def sample(L, r, c, log_floor=-np.inf):
    """The Catmull-Rom interpolant of L [H, W] at cells (r, c), arrays of one shape with 0 <= r <= H - 1 and 0 <= c <= W - 1; log_floor
    where none of the 16 taps lies above log_floor."""
    H, W = L.shape
    fr, fc = np.floor(r), np.floor(c)
    wr, wc = weights(r - fr), weights(c - fc)
    ir, ic = fr.astype(np.int64), fc.astype(np.int64)
    total, above = None, False
    for a in range(4):
        ra = np.clip(ir - 1 + a, 0, H - 1)
        row = None
        for b in range(4):
            l = L[ra, np.clip(ic - 1 + b, 0, W - 1)]
            above = above | (l > log_floor)
            t = wc[b] * l
            row = t if row is None else row + t
        t = wr[a] * row
        total = t if total is None else total + t
    return np.where(above, total, log_floor)


def view_term(L, P, flip, X, cell, log_floor):
    """What one view adds to the score of the points X [..., 3]."""
    H, W = L.shape
    row_px, col_px, w = project(P, X)
    r, c = to_cells(row_px, col_px, flip, cell, W)
    with np.errstate(invalid="ignore"):
        ok = (w > 0.0) & (r >= 0.0) & (r <= H - 1.0) & (c >= 0.0) & (c <= W - 1.0)
    s = sample(L, np.where(ok, r, 0.0), np.where(ok, c, 0.0), log_floor)
    return np.where(ok & (s > log_floor), s, log_floor)


class Logs:
    """The l planes of hm [n, V, C, H, W], computed once each."""

    def __init__(self, hm, floor):
        self.hm, self.floor, self.log_floor, self.cache = hm, float(floor), float(np.log(floor)), {}

    def __call__(self, t, v, p):
        key = (t, v, p)
        if key not in self.cache:
            self.cache[key] = cell_logs(self.hm[t, v, p], self.floor, self.log_floor)
        return self.cache[key]


def cell_size(image_shape, H, W):
    """(rows, cols) pixels per cell; image_shape is the project's [W, H] = (columns, rows) of the camera images."""
    return float(image_shape[1]) / H, float(image_shape[0]) / W


def scores(hm, P, flip, plane, pts, image_shape, floor):
    """score [n, J, M] of the points pts [n, J, M, 3]."""
    n, V, C, H, W = hm.shape
    J = plane.shape[1]
    cell, logs = cell_size(image_shape, H, W), Logs(hm, floor)
    out = np.zeros(pts.shape[:3], dtype=np.float64)
    for t in range(n):
        for j in range(J):
            s = np.zeros(pts.shape[2], dtype=np.float64)
            for v in range(V):
                if plane[v, j] >= 0:
                    s = s + view_term(logs(t, v, int(plane[v, j])), P[v], bool(flip[v]), pts[t, j], cell, logs.log_floor)
            out[t, j] = s
    return out


def _grid_points(centre, step):
    g = [centre[a] + _OFF * step for a in range(3)]
    X = np.empty((GRID, GRID, GRID, 3), dtype=np.float64)
    X[..., 0], X[..., 1], X[..., 2] = g[0][:, None, None], g[1][None, :, None], g[2][None, None, :]
    return X.reshape(-1, 3)


def triangulate(hm, P, flip, plane, X0, image_shape, half, levels, floor):
    """dict of points [n, J, 3], score, status (int8), views (int32), shift, choice [n, J, levels] (int32), counts [J, 4] (int64) and
    gap [n, J, levels]: the best score minus the second best of every level searched (+inf elsewhere); ties [n, J, levels] (int32): how
    many of the level's 512 scores equal the best (0 elsewhere); gap_next: the best score minus the largest score strictly below it
    (+inf elsewhere, and where all 512 are equal)."""
    n, V, C, H, W = hm.shape
    J = plane.shape[1]
    cell, logs = cell_size(image_shape, H, W), Logs(hm, floor)
    lf = logs.log_floor
    X = np.array(X0, dtype=np.float64, copy=True)
    score = np.full((n, J), np.nan)
    status = np.zeros((n, J), dtype=np.int8)
    views = np.zeros((n, J), dtype=np.int32)
    shift = np.zeros((n, J), dtype=np.float64)
    choice = np.full((n, J, levels), -1, dtype=np.int32)
    gap = np.full((n, J, levels), np.inf)
    gap_next = np.full((n, J, levels), np.inf)
    ties = np.zeros((n, J, levels), dtype=np.int32)
    for t in range(n):
        for j in range(J):
            vs = [v for v in range(V) if plane[v, j] >= 0]
            views[t, j] = sum(1 << v for v in vs)
            x0 = X0[t, j]
            if len(vs) < 2 or not np.isfinite(x0).all() or not x0.any():
                continue
            base = 0.0
            for _ in vs:
                base = base + lf
            centre, h = x0.copy(), float(half)
            for level in range(levels):
                step = 2.0 * h / GRID
                pts = _grid_points(centre, step)
                s = np.zeros(len(pts), dtype=np.float64)
                for v in vs:
                    s = s + view_term(logs(t, v, int(plane[v, j])), P[v], bool(flip[v]), pts, cell, lf)
                best = int(np.argmax(s))   # the first of equals
                if level == 0:
                    if not s[best] > base:
                        status[t, j], score[t, j] = 2, s[best]
                        break
                    i = np.array([best // 64, best // 8 % 8, best % 8])
                    status[t, j] = 3 if ((i == 0) | (i == GRID - 1)).any() else 1
                top = np.sort(s)[-2:]
                gap[t, j, level] = top[1] - top[0]
                ties[t, j, level] = (s == s[best]).sum()
                below = s[s < s[best]]
                if below.size:
                    gap_next[t, j, level] = s[best] - below.max()
                choice[t, j, level] = best
                centre, h, score[t, j] = pts[best].copy(), step, s[best]
            if status[t, j] != 2:
                X[t, j] = centre
                d = centre - x0
                shift[t, j] = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    counts = np.stack([(status == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int64)
    return dict(points=X, score=score, status=status, views=views, shift=shift, choice=choice, counts=counts, gap=gap, ties=ties,
                gap_next=gap_next)


REACH = 1.25   # the cube a search can reach, in half widths of its first level


def windows(P, flip, plane, X0, image_shape, H, W, half):
    """(used [n, J] int64, win [n, J, V, 4] int64) of the window rule: per view of a searched (frame, joint) the cells (r0, r1, c0, c1)
    the kernel would stage -- the bounding box of the 8 corners X0 +- 1.25 half in cells, floor(min) - 1 .. floor(max) + 2, clamped to the
    plane; the whole plane where some but not all corners have w <= 0 or a corner's w, r or c is not finite; (0, -1, 0, -1), no window,
    where all 8 have w <= 0, and for a view without a plane -- and the number of cells of the joint's windows together, 0 for a
    (frame, joint) that is not searched."""
    n, J = X0.shape[:2]
    V = len(P)
    cell = cell_size(image_shape, H, W)
    used = np.zeros((n, J), dtype=np.int64)
    win = np.tile(np.array([0, -1, 0, -1], dtype=np.int64), (n, J, V, 1))
    e = float(half) * REACH
    sign = np.array([[1.0 if k & 4 else -1.0, 1.0 if k & 2 else -1.0, 1.0 if k & 1 else -1.0] for k in range(8)])
    for t in range(n):
        for j in range(J):
            vs = [v for v in range(V) if plane[v, j] >= 0]
            x0 = X0[t, j]
            if len(vs) < 2 or not np.isfinite(x0).all() or not x0.any():
                continue
            corners = x0[None, :] + sign * e
            for v in vs:
                row_px, col_px, w = project(P[v], corners)
                r, c = to_cells(row_px, col_px, bool(flip[v]), cell, W)
                finite = np.isfinite(w) & np.isfinite(r) & np.isfinite(c)
                behind = int((finite & ~(w > 0.0)).sum())
                if finite.all() and behind == 8:
                    continue
                if not finite.all() or behind > 0:
                    box = (0, H - 1, 0, W - 1)
                else:
                    box = (int(min(max(np.floor(r.min()) - 1.0, 0.0), H - 1.0)), int(min(max(np.floor(r.max()) + 2.0, 0.0), H - 1.0)),
                           int(min(max(np.floor(c.min()) - 1.0, 0.0), W - 1.0)), int(min(max(np.floor(c.max()) + 2.0, 0.0), W - 1.0)))
                win[t, j, v] = box
                used[t, j] += (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
    return used, win


def taps(hm_plane, P, flip, X, cell):
    """What the sampler reads for the points X [M, 3] in one view: (ok [M] bool: the view informs, f [M, 2]: the fractions
    (r - floor(r), c - floor(c)), cells [M, 16] float32: the plane's values at the 16 taps, rows outside, in the sampler's order)."""
    H, W = hm_plane.shape
    row_px, col_px, w = project(P, X)
    r, c = to_cells(row_px, col_px, flip, cell, W)
    with np.errstate(invalid="ignore"):
        ok = (w > 0.0) & (r >= 0.0) & (r <= H - 1.0) & (c >= 0.0) & (c <= W - 1.0)
    r, c = np.where(ok, r, 0.0), np.where(ok, c, 0.0)
    fr, fc = np.floor(r), np.floor(c)
    ir, ic = fr.astype(np.int64), fc.astype(np.int64)
    rows = np.clip(ir[:, None] - 1 + np.arange(4)[None, :], 0, H - 1)
    cols = np.clip(ic[:, None] - 1 + np.arange(4)[None, :], 0, W - 1)
    return ok, np.stack([r - fr, c - fc], axis=1), hm_plane[rows[:, :, None], cols[:, None, :]].reshape(len(X), 16)


# ---- planted inputs -----------------------------------------------------------------------------------------------------------------
def blob_maps(P, flip, plane, X, image_shape, C, H=64, W=128, sigma=1.0, second=None, noise=0.0, seed=0, long=()):
    """hm [n, V, C, H, W] float32: a Gaussian blob (deviation `sigma` cells, or (rows, cols)) at the projection of X [n, J, 3] in the plane
    of every view of every joint.  `second`: (view or views, amplitude, (d_rows, d_cols)) adds a blob of that amplitude beside the true one in
    those views.  `noise`: the deviation of Gaussian noise added to every cell.  `long`: the views whose blobs are four times as long along
    the columns."""
    n, J = X.shape[:2]
    V = len(P)
    cell = cell_size(image_shape, H, W)
    rr, cc = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    sr, sc = (sigma, sigma) if np.isscalar(sigma) else sigma
    hm = np.zeros((n, V, C, H, W), dtype=np.float64)
    for v in range(V):
        sc = (sigma if np.isscalar(sigma) else sigma[1]) * (4.0 if v in long else 1.0)
        for j in range(J):
            if plane[v, j] < 0:
                continue
            row_px, col_px, _ = project(P[v], X[:, j])
            r, c = to_cells(row_px, col_px, bool(flip[v]), cell, W)
            for t in range(n):
                g = np.exp(-0.5 * (((rr - r[t]) / sr) ** 2 + ((cc - c[t]) / sc) ** 2))
                if second is not None and v in np.atleast_1d(second[0]):
                    g = g + second[1] * np.exp(-0.5 * (((rr - r[t] - second[2][0]) / sr) ** 2 + ((cc - c[t] - second[2][1]) / sc) ** 2))
                hm[t, v, plane[v, j]] = g
    if noise:
        hm += np.random.default_rng(seed).normal(0.0, noise, hm.shape)
    return hm.astype(np.float32)


def argmax_dlt(hm, P, flip, plane, image_shape):
    """The arg-max of every plane, un-flipped and scaled to pixels as the project does, and the DLT of the joint's views: [n, J, 3]."""
    n, V, C, H, W = hm.shape
    J = plane.shape[1]
    cell = cell_size(image_shape, H, W)
    X = np.zeros((n, J, 3))
    for t in range(n):
        for j in range(J):
            rows = []
            for v in range(V):
                if plane[v, j] < 0:
                    continue
                r, c = np.unravel_index(int(np.argmax(hm[t, v, plane[v, j]])), (H, W))
                y, x = r * cell[0], ((W - c) if flip[v] else c) * cell[1]
                rows += [x * P[v][2] - P[v][0], y * P[v][2] - P[v][1]]
            if len(rows) >= 4:
                e = np.linalg.svd(np.array(rows))[2][-1]
                X[t, j] = e[:3] / e[3]
    return X
