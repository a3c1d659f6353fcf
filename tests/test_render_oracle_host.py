"""CPU: oracle/render.py, the numpy restatement that tests/test_gpu_video.py and tests/test_gpu_render_sweep.py compare the drawing
kernels of csrc/render.hip with bit for bit, checked on its own.

The oracle is vectorised (masks over whole images, fancy indexing for the resize taps); a slip there would be copied into every GPU
comparison.  Here the documented rule is stated a second time, one pixel at a time in plain Python floats (IEEE doubles, no fused
multiply-add: the arithmetic of both the kernels and numpy), on frames of about 9 x 13, and compared bit for bit; then properties that
need no second statement at all: the lattice points of a disc, identity and constant resizes, and the table order of bones.

The rule (csrc/render.hip, include/df3d_hip.h):
  pose2d  a pixel shows its camera's grey value; then every bone (a, b) of the table, in order, whose two joints are seen (neither
          coordinate is exactly 0) and whose segment lies within line_width / 2 of the pixel, paints joint a's colour; then every seen
          joint, in order, within `radius` of the pixel paints its own.  Distances are squared and compared with <=.
  pose3d  joints are projected orthographically (azimuth, elevation in degrees), +-lim onto [0, size - 1]; bones as above on black.
  resize  bilinear, pixel centres at half integers, source coordinate clamped to the image, floor(v + 0.5).
"""
import math

import numpy as np
import pytest

from oracle import render as orr

H, W = 9, 13


# ---- the rule, one pixel at a time ---------------------------------------------------------------------------------------------------
def seg_dist2(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    len2 = dx * dx + dy * dy
    t = ((px - ax) * dx + (py - ay) * dy) / len2 if len2 > 0.0 else 0.0
    if t < 0.0:
        t = 0.0
    elif t > 1.0:
        t = 1.0
    qx, qy = ax + t * dx, ay + t * dy
    return (px - qx) * (px - qx) + (py - qy) * (py - qy)


def pixel2d(grey, y, x, pts, bones, rgb, radius, line_width):
    colour = (grey, grey, grey)
    half = 0.5 * line_width
    for a, b in bones:
        if pts[a][0] == 0.0 or pts[a][1] == 0.0 or pts[b][0] == 0.0 or pts[b][1] == 0.0:
            continue
        if seg_dist2(float(x), float(y), pts[a][1], pts[a][0], pts[b][1], pts[b][0]) <= half * half:
            colour = tuple(rgb[a])
    for j, (row, col) in enumerate(pts):
        if row == 0.0 or col == 0.0:
            continue
        dx, dy = float(x) - col, float(y) - row
        if dx * dx + dy * dy <= radius * radius:
            colour = tuple(rgb[j])
    return colour


def scalar_pose2d(luma, points, bones, rgb, radius, line_width):
    _, h, w = luma.shape
    out = np.zeros((2 * h, 3 * w, 3), np.uint8)
    for slot in range(6):
        pts = [(float(r), float(c)) for r, c in points[slot]]
        for y in range(h):
            for x in range(w):
                out[(slot // 3) * h + y, (slot % 3) * w + x] = pixel2d(int(luma[slot, y, x]), y, x, pts, bones, rgb, radius, line_width)
    return out


def scalar_pose3d(points3d, bones, rgb, az3, elev, lim, size, line_width):
    out = np.zeros((size, 3 * size, 3), np.uint8)
    k = math.pi / 180.0
    ce, se = math.cos(elev * k), math.sin(elev * k)
    half = 0.5 * line_width
    for panel in range(3):
        ca, sa = math.cos(az3[panel] * k), math.sin(az3[panel] * k)
        screen = []
        for X, Y, Z in ((float(a), float(b), float(c)) for a, b, c in points3d):
            u = -sa * X + ca * Y
            v = -se * ca * X - se * sa * Y + ce * Z
            screen.append(((u / lim * 0.5 + 0.5) * float(size - 1), (0.5 - v / lim * 0.5) * float(size - 1)))
        for y in range(size):
            for x in range(size):
                for a, b in bones:
                    if seg_dist2(float(x), float(y), screen[a][0], screen[a][1], screen[b][0], screen[b][1]) <= half * half:
                        out[y, panel * size + x] = rgb[a]
    return out


def scalar_resize(img, oh, ow, unrounded=False):
    ih, iw = img.shape[:2]
    out = np.zeros((oh, ow, 3), np.float64 if unrounded else np.uint8)
    for y in range(oh):
        for x in range(ow):
            fy = (y + 0.5) * float(ih) / float(oh) - 0.5
            fx = (x + 0.5) * float(iw) / float(ow) - 0.5
            cy, cx = min(max(fy, 0.0), float(ih - 1)), min(max(fx, 0.0), float(iw - 1))
            y0, x0 = int(math.floor(cy)), int(math.floor(cx))
            y1, x1 = min(y0 + 1, ih - 1), min(x0 + 1, iw - 1)
            wy, wx = cy - y0, cx - x0
            for c in range(3):
                v00, v01, v10, v11 = (float(img[yy, xx, c]) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
                top = v00 + wx * (v01 - v00)
                bot = v10 + wx * (v11 - v10)
                v = top + wy * (bot - top)
                out[y, x, c] = v if unrounded else int(math.floor(v + 0.5))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def distinct_colours(rng, n):
    """n pairwise distinct RGB triples, none of them grey (a grey one could pass for the camera image)."""
    seen, out = set(), []
    while len(out) < n:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if c not in seen and not (c[0] == c[1] == c[2]):
            seen.add(c)
            out.append(c)
    return np.asarray(out, np.uint8)


def quarter_points(rng, shape, h, w):
    """(row, col) on quarter-pixel positions in [-10, h + 10] x [-10, w + 10], never exactly 0."""
    rows = rng.integers(-40, 4 * (h + 10) + 1, shape) / 4.0
    cols = rng.integers(-40, 4 * (w + 10) + 1, shape) / 4.0
    rows[rows == 0.0] = 0.25
    cols[cols == 0.0] = 0.25
    return np.stack([rows, cols], axis=-1)


@pytest.mark.parametrize("radius,line_width", [(0.0, 0.0), (0.5, 1.0), (3.0, 2.5), (1.0, 0.0), (0.0, 2.5)])
def test_pose2d_grid_equals_the_pixel_by_pixel_rule(radius, line_width):
    rng = np.random.default_rng(int(radius * 10 + line_width * 100))
    J = 12
    luma = rng.integers(0, 256, (6, H, W), dtype=np.uint8)
    pts = quarter_points(rng, (6, J), H, W)
    pts[:, :6] = np.stack([rng.integers(1, 4 * H, (6, 6)), rng.integers(1, 4 * W, (6, 6))], axis=-1) / 4.0   # half of the joints inside the frame
    pts[0, 1] = pts[0, 0]                      # coincident joints: the bone (0, 1) is a point
    pts[1, 2, 0], pts[1, 3, 1] = 0.0, 0.0      # unseen by the row alone, by the column alone
    pts[2, 4] = (3.0, 4.0)                     # on a pixel
    pts[3, 0, 0], pts[3, 1, 1], pts[3, 2, 0], pts[3, 3] = np.nan, np.inf, -np.inf, (1e300, 1e300)
    bones = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (7, 7), (4, 4), (2, 9), (0, 3), (6, 11), (5, 1)]
    rgb = distinct_colours(rng, J)
    got = orr.pose2d_grid(luma, pts, bones, rgb, radius, line_width)
    ref = scalar_pose2d(luma, pts, bones, rgb, radius, line_width)
    assert got.shape == (2 * H, 3 * W, 3) and got.dtype == np.uint8 and np.array_equal(got, ref)
    grey = np.concatenate([np.concatenate(list(luma[:3]), 1), np.concatenate(list(luma[3:]), 1)], 0)
    assert (got != grey[:, :, None]).any(), "nothing was drawn: the comparison is one of grey images"


@pytest.mark.parametrize("size,lim,elev,line_width", [(9, 2.0, 30.0, 1.5), (13, 2.0, 0.0, 0.0), (8, 1e-3, 90.0, 1.5), (9, 1e6, -30.0, 1e9), (2, 2.0, 30.0, 1.5)])
def test_pose3d_panels_equal_the_pixel_by_pixel_rule(size, lim, elev, line_width):
    rng = np.random.default_rng(size)
    J = 10
    p3 = rng.uniform(-3.0, 3.0, (J, 3))
    p3[7, 1] = np.nan
    bones = [(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 8), (8, 9), (9, 9), (4, 0)]
    rgb = distinct_colours(rng, J)
    az = [0.0, -60.0, 405.0] if size % 2 else [90.0, 120.0, 210.0]
    got = orr.pose3d_panels(p3, bones, rgb, az, elev, lim, size, line_width)
    ref = scalar_pose3d(p3, bones, rgb, az, elev, lim, size, line_width)
    assert got.shape == (size, 3 * size, 3) and np.array_equal(got, ref)
    if line_width >= 1.0 and lim == 2.0:
        assert got.any()


@pytest.mark.parametrize("src,dst", [((9, 13), (9, 13)), ((9, 13), (4, 5)), ((4, 5), (9, 13)), ((1, 1), (5, 7)), ((3, 5), (1, 1)), ((9, 13), (18, 26)), ((2, 13), (3, 7))])
def test_resize_rgb_equals_the_pixel_by_pixel_rule(src, dst):
    rng = np.random.default_rng(src[0] * 100 + dst[1])
    img = rng.integers(0, 256, (*src, 3), dtype=np.uint8)
    assert np.array_equal(orr.resize_rgb(img, *dst), scalar_resize(img, *dst))
    raw = orr.resize_rgb(img, *dst, unrounded=True)
    assert raw.dtype == np.float64 and np.array_equal(raw, scalar_resize(img, *dst, unrounded=True))
    assert np.array_equal(np.floor(raw + 0.5).astype(np.uint8), orr.resize_rgb(img, *dst))


def test_resize_rounds_a_half_up():
    """A 2x up-scale of columns that rise by 2: the taps' weights are 1/4 and 3/4, so every interior pixel lies on k + 0.5 exactly."""
    img = np.zeros((4, 8, 3), np.uint8)
    img[:] = (2 * np.arange(8, dtype=np.uint8))[None, :, None] + np.arange(3, dtype=np.uint8)[None, None, :] * 40
    raw = orr.resize_rgb(img, 4, 16, unrounded=True)
    halves = raw - np.floor(raw) == 0.5
    assert halves.sum() >= 100
    out = orr.resize_rgb(img, 4, 16)
    assert np.array_equal(out[halves], (raw[halves] + 0.5).astype(np.uint8)) and np.array_equal(out, scalar_resize(img, 4, 16))


# ---- properties that need no second statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius4", [0, 2, 4, 10, 12, 17])   # radius in quarter pixels: 0, 0.5, 1, 2.5, 3, 4.25
def test_a_disc_colours_exactly_its_lattice_points(radius4):
    luma = np.full((6, H, W), 7, np.uint8)
    pts = np.zeros((6, 1, 2))
    pts[:] = (4.0, 6.0)
    got = orr.pose2d_grid(luma, pts, [], np.asarray([[200, 10, 30]], np.uint8), radius4 / 4.0, 0.0)[:H, :W]
    want = np.array([[16 * ((y - 4) ** 2 + (x - 6) ** 2) <= radius4 ** 2 for x in range(W)] for y in range(H)])   # integers only
    assert np.array_equal((got == (200, 10, 30)).all(2), want) and np.array_equal((got == 7).all(2), ~want)
    assert want.sum() == {0: 1, 2: 1, 4: 5, 10: 21, 12: 29, 17: 61}[radius4]   # the Gauss circle counts


@pytest.mark.parametrize("src,dst", [((9, 13), (9, 13)), ((1, 1), (1, 1)), ((1, 13), (1, 13))])
def test_an_identity_resize_returns_its_input(src, dst):
    img = np.random.default_rng(3).integers(0, 256, (*src, 3), dtype=np.uint8)
    assert np.array_equal(orr.resize_rgb(img, *dst), img)


@pytest.mark.parametrize("dst", [(9, 13), (4, 5), (20, 31), (1, 1), (1, 40)])
def test_a_constant_image_resizes_to_the_same_constant(dst):
    img = np.empty((9, 13, 3), np.uint8)
    img[:] = (0, 255, 113)
    out = orr.resize_rgb(img, *dst)
    assert out.shape == (*dst, 3) and (out == (0, 255, 113)).all()


def _two_bone_frame(bones):
    """Joints off the lattice and radius 0: no disc is drawn, only the bones show."""
    luma = np.full((6, H, W), 9, np.uint8)
    pts = np.zeros((6, 6, 2))
    pts[:] = [(1.25, 1.25), (7.25, 11.25), (7.25, 1.25), (1.25, 11.25), (0.25, 3.25), (0.25, 9.25)]
    rgb = np.asarray([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)], np.uint8)
    masks = dict(orr.pose2d_masks(H, W, pts[0], bones, 0.0, 2.0)[0])
    return orr.pose2d_grid(luma, pts, bones, rgb, 0.0, 2.0)[:H, :W], masks


def test_the_order_of_two_bones_matters_exactly_where_they_overlap():
    # the two diagonals cross; the short bone along the top row touches neither of them
    crossing, apart = [(0, 1), (2, 3)], [(2, 3), (4, 5)]
    a, masks = _two_bone_frame(crossing)
    b, _ = _two_bone_frame(crossing[::-1])
    overlap = masks[0] & masks[1]
    assert overlap.sum() >= 3 and np.array_equal((a != b).any(2), overlap)
    assert (a[overlap] == (0, 0, 255)).all() and (b[overlap] == (255, 0, 0)).all()   # the later entry wins, with its FIRST joint's colour
    c, masks = _two_bone_frame(apart)
    d, _ = _two_bone_frame(apart[::-1])
    assert masks[0].any() and masks[1].any() and not (masks[0] & masks[1]).any() and np.array_equal(c, d)
