"""Float64 numpy statement of the sub-pixel localisation of heat-map peaks.  This module DEFINES the rule
the device kernels (deepfly3d_amd/csrc/subpixel_dev.h) implement; the reference has no such step and no other implementation is
involved.  Test infrastructure only (not collected: no test_ prefix); numpy alone.

The order of the float64 operations below is part of the rule: the kernels are compiled without multiply-add fusion and are compared
with this module bit for bit.
"""
import numpy as np

# the branch refine_cell took, for the tests of the rule itself
BORDER, NONFINITE, NEWTON, PER_AXIS = "border", "nonfinite", "newton", "per_axis"


def _axis(g, h):
    """One axis alone: the clamped Newton step of the 1-D quadratic, 0 where it has no maximum."""
    if not h < 0.0:
        return np.float64(0.0)
    d = -(g / h)
    return np.float64(min(max(d, -0.5), 0.5))


def refine_cell(plane, r, c):
    """plane [H, W] float32, (r, c) a cell -> (dy, dx, branch): the offset of the peak from the cell centre, each in [-0.5, 0.5]."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    zero = np.float64(0.0)
    if r == 0 or r == H - 1 or c == 0 or c == W - 1:
        return zero, zero, BORDER
    n = plane[r - 1 : r + 2, c - 1 : c + 2].astype(np.float64)   # n[1 + dy, 1 + dx]
    if not np.all(np.isfinite(n)):
        return zero, zero, NONFINITE
    gy = 0.5 * (n[2, 1] - n[0, 1])
    gx = 0.5 * (n[1, 2] - n[1, 0])
    hyy = (n[2, 1] - 2.0 * n[1, 1]) + n[0, 1]
    hxx = (n[1, 2] - 2.0 * n[1, 1]) + n[1, 0]
    hxy = 0.25 * (((n[2, 2] - n[2, 0]) - n[0, 2]) + n[0, 0])
    det = hxx * hyy - hxy * hxy
    if hxx < 0.0 and hyy < 0.0 and det > 0.0:
        dx = -((hyy * gx - hxy * gy) / det)
        dy = -((hxx * gy - hxy * gx) / det)
        if abs(dx) <= 0.5 and abs(dy) <= 0.5:
            return dy, dx, NEWTON
    return _axis(gy, hyy), _axis(gx, hxx), PER_AXIS


def refine_point(plane, r, c):
    """The refined normalised point of cell (r, c): float32((r + dy) * (1 / H)), float32((c + dx) * (1 / W)), sums and products in
    float64, one rounding at the end (H, W powers of two)."""
    H, W = np.asarray(plane).shape
    dy, dx, _ = refine_cell(plane, r, c)
    return np.float32((np.float64(r) + dy) * (1.0 / H)), np.float32((np.float64(c) + dx) * (1.0 / W))


def argmax_cells(hm):
    """hm [n, J, H, W] float32 -> (rows, cols) [n, J] of the arg-max cell as df3d_heatmap_argmax picks it: the first index of the largest
    value in row-major order, a NaN never wins, and a plane without any value above -inf resolves to cell 0."""
    hm = np.asarray(hm, np.float32)
    n, J, H, W = hm.shape
    flat = hm.reshape(n, J, H * W)
    idx = np.where(np.isnan(flat), -np.inf, flat).argmax(axis=-1)
    return idx // W, idx % W


def heatmap_argmax_subpixel(hm):
    """hm [n, J, H, W] float32 -> points [n, J, 2] float32 (refined row / H, col / W), conf [n, J] float32 (the value of the cell)."""
    hm = np.asarray(hm, np.float32)
    n, J, H, W = hm.shape
    rows, cols = argmax_cells(hm)
    pts = np.zeros((n, J, 2), np.float32)
    conf = np.zeros((n, J), np.float32)
    for a in range(n):
        for b in range(J):
            pts[a, b] = refine_point(hm[a, b], int(rows[a, b]), int(cols[a, b]))
            conf[a, b] = hm[a, b, rows[a, b], cols[a, b]]
    return pts, conf


def refine_peaks(hm, count, cell_pts):
    """hm [n, J, H, W]; count [n, J] and cell_pts [n, J, K, 2] float32 (row / H, col / W) as df3d_heatmap_peaks reports them -> the
    refined points [n, J, K, 2] float32 of the same cells; unused slots zero."""
    hm = np.asarray(hm, np.float32)
    n, J, H, W = hm.shape
    out = np.zeros_like(np.asarray(cell_pts, np.float32))
    for a in range(n):
        for b in range(J):
            for s in range(int(count[a, b])):
                r, c = int(round(float(cell_pts[a, b, s, 0]) * H)), int(round(float(cell_pts[a, b, s, 1]) * W))
                out[a, b, s] = refine_point(hm[a, b], r, c)
    return out


def gaussian_plane(center_row, center_col, sigma, shape=(64, 128)):
    """A float32 Gaussian heat-map of unit height centred at (center_row, center_col) in cells (cell centres at the integers)."""
    r = np.arange(shape[0], dtype=np.float64)[:, None]
    c = np.arange(shape[1], dtype=np.float64)[None, :]
    return np.exp(-((r - center_row) ** 2 + (c - center_col) ** 2) / (2.0 * sigma * sigma)).astype(np.float32)
