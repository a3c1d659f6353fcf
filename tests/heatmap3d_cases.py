"""Seeded inputs for the heat-map triangulation (csrc/heatmap3d.hip): Gaussian blobs planted at the projections of
3-D points under the golden calibration.  Host numpy only; every case and its oracle result is computed once and read only.
TEST INFRASTRUCTURE ONLY."""
import functools
import os

import numpy as np

import heatmap3d_oracle as ho

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGE_SHAPE = (960, 480)   # [W, H] of the golden recording's images
H, W = 64, 128
HALF, LEVELS, FLOOR = 0.4, 4, 1e-3   # config.HEATMAP3D_*
PLANT_MM = 0.02
GAP = 1e-9                 # a level whose two best scores lie closer than this is not compared (at most MAX_SKIPPED of a test's cases)
MAX_SKIPPED = 0.01


@functools.lru_cache(maxsize=None)
def golden():
    """(P [7, 3, 4], pose [15, 38, 3]) of the golden recording."""
    g3 = np.load(os.path.join(GOLDEN, "golden_3d.npz"))
    P = np.stack([g3["intr"][c] @ np.concatenate([g3["R"][c], g3["tvec"][c][:, None]], axis=1) for c in range(7)])
    return np.ascontiguousarray(P, dtype=np.float64), g3["points3d_wo_procrustes"].astype(np.float64)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def fly(n=2, noise=0.0, second=False, views=0, sigma=1.0, seed=0, long=False):
    """The fly layout: the six cameras with planes, 38 joints, `n` golden frames; the planted points are the pose + N(0, 0.02 mm) and the
    search starts at the pose.  `views` = 2 drops the middle camera of each side, 3 keeps the joints that three cameras see (30 of 38).
    `second`: the first view of every joint carries a 1.3 x stronger second blob 6 cells away; `long`: its blob is 4 cells long.  dict of hm, P, flip, plane, X0, planted."""
    from deepfly3d_amd.heatmap3d import view_table

    P7, pose = golden()
    cameras, flip, plane = view_table()
    plane = plane.copy()
    if views == 2:
        plane[[1, 4]] = -1
    if views == 3:
        plane = plane[:, (plane >= 0).sum(axis=0) == 3]
    joints = np.arange(38) if views != 3 else np.nonzero((view_table()[2] >= 0).sum(axis=0) == 3)[0]
    X0 = np.ascontiguousarray(pose[:n][:, joints])
    planted = X0 + np.random.default_rng([seed, n]).normal(0.0, PLANT_MM, X0.shape)
    extra = ((0, 3), 1.3, (0.0, 6.0)) if second else None
    hm = ho.blob_maps(P7[cameras], flip, plane, planted, IMAGE_SHAPE, 19, H, W, sigma=sigma, second=extra, noise=noise, seed=seed, long=(0, 3) if long else ())
    return _frozen(dict(hm=hm, P=np.ascontiguousarray(P7[cameras]), flip=flip, plane=np.ascontiguousarray(plane), X0=X0, planted=planted))


def _shifted(P, d_rows, d_cols):
    """P with every projection moved by (d_rows, d_cols) pixels."""
    T = np.array([[1.0, 0.0, d_cols], [0.0, 1.0, d_rows], [0.0, 0.0, 1.0]])
    return T @ P


@functools.lru_cache(maxsize=None)
def special(V):
    """n = 3, J = 4, C = 5, V in (2, 3, 8) views taken from eight: 0 plain, 1 plain and flipped, 2 .. 5 moved so that one of the joints lies
    0.6 cell inside the top, bottom, left and right (flipped) edge of the plane, where the window and the taps are clamped, 6 behind the
    camera (w <= 0 everywhere: it says nothing), 7 plain.  Joint 3 has a plane in view 0 only (status 0).  Frame 0: the search of joint 2 starts 0.37 mm beside the pose (status 3).  Frame 1: X0 of joint 0 is
    zero and of joint 1 holds a NaN (status 0).  Frame 2: joint 0's planes are all zero (status 2) and joint 1's hold a NaN, an infinity
    and a negative cell beside the blob."""
    P7, pose = golden()
    n, J, C = 3, 4, 5
    X0 = np.ascontiguousarray(pose[:n, :J])
    planted = X0 + np.random.default_rng([7, V]).normal(0.0, PLANT_MM, X0.shape)
    cell = ho.cell_size(IMAGE_SHAPE, H, W)

    def edge(P, flip, side):
        row_px, col_px, _ = ho.project(P, planted[:, :3])
        r, c = ho.to_cells(row_px, col_px, flip, cell, W)
        if side == "top":
            return _shifted(P, (0.6 - r.min()) * cell[0], 0.0)
        if side == "bottom":
            return _shifted(P, (H - 1.6 - r.max()) * cell[0], 0.0)
        if side == "left":
            return _shifted(P, 0.0, (0.6 - c.min()) * cell[1])
        return _shifted(P, 0.0, (c.max() - (W - 1.6)) * cell[1])   # a flipped view: its cell columns run against the pixels

    eight = [(P7[0], 0), (P7[1], 1), (edge(P7[2], False, "top"), 0), (edge(P7[0], False, "bottom"), 0), (edge(P7[1], False, "left"), 0),
             (edge(P7[2], True, "right"), 1), (-P7[0], 0), (P7[1], 0)]
    pick = {2: (0, 2), 3: (1, 3, 5), 8: tuple(range(8))}[V]
    P = np.ascontiguousarray(np.stack([eight[k][0] for k in pick]))
    flip = np.array([eight[k][1] for k in pick], dtype=np.uint8)
    plane = np.array([[(v + j) % C for j in range(J)] for v in range(V)], dtype=np.int32)
    plane[1:, 3] = -1
    hm = ho.blob_maps(P, flip, plane, planted, IMAGE_SHAPE, C, H, W).copy()
    X0[0, 2, 0] += 0.37   # the blob lies in the outermost layer of the first cube (status 3); the search follows it
    X0[1, 0] = 0.0
    X0[1, 1, 1] = np.nan
    for v in range(V):
        hm[2, v, plane[v, 0]] = 0.0
        row_px, col_px, _ = ho.project(P[v], planted[2, 1])
        r, c = ho.to_cells(row_px, col_px, bool(flip[v]), cell, W)
        if 2.0 <= r <= H - 3.0 and 2.0 <= c <= W - 3.0:
            hm[2, v, plane[v, 1], int(r) + 2, int(c)] = np.nan
            hm[2, v, plane[v, 1], int(r), int(c) + 2] = np.inf
            hm[2, v, plane[v, 1], int(r) - 1, int(c) - 1] = -1.0
    return _frozen(dict(hm=hm, P=P, flip=flip, plane=plane, X0=X0, planted=planted))


@functools.lru_cache(maxsize=None)
def ortho(seed=0):
    """Two views whose cells are coordinates of the point itself, exactly: view 0 has column = x and row = y, view 1 (flipped) column =
    W - x and row = z, both with w = 1.  n = 1, J = 2, C = 2, planes of uniform noise with cells at and below the floor.  The points:
    every combination of x in (0, 0.5, 1, 63.25, 127, 128, -0.001, 127.001), y and z in (0, 0.75, 31.5, 63, -0.001, 63.001) -- on the four
    edges exactly, just outside them, inside -- and 64 uniform ones.  dict of hm, P, flip, plane, pts [1, 2, M, 3]."""
    rng = np.random.default_rng(seed)
    cell = ho.cell_size(IMAGE_SHAPE, H, W)
    P = np.zeros((2, 3, 4))
    P[0, 0, 0], P[0, 1, 1], P[0, 2, 3] = cell[1], cell[0], 1.0
    P[1, 0, 0], P[1, 1, 2], P[1, 2, 3] = cell[1], cell[0], 1.0
    hm = rng.uniform(0.0, 1.0, (1, 2, 2, H, W)).astype(np.float32)
    hm[hm < 0.05] = FLOOR / 2
    hm[0, 0, 0, 0, 0] = np.float32(FLOOR)   # the float32 nearest to the floor lies above or below it: either way one rule decides
    xs, ys = (0.0, 0.5, 1.0, 63.25, 127.0, 128.0, -0.001, 127.001), (0.0, 0.75, 31.5, 63.0, -0.001, 63.001)
    grid = np.array([(x, y, z) for x in xs for y in ys for z in ys])
    rand = rng.uniform((0.0, 0.0, 0.0), (127.0, 63.0, 63.0), (64, 3))
    pts = np.concatenate([grid, rand])
    pts = np.ascontiguousarray(np.broadcast_to(pts, (1, 2, *pts.shape)))
    return _frozen(dict(hm=hm, P=P, flip=np.array([0, 1], dtype=np.uint8), plane=np.array([[0, 1], [1, 0]], dtype=np.int32), pts=pts))


@functools.lru_cache(maxsize=None)
def reference(name, *args, half=HALF, levels=LEVELS, floor=FLOOR):
    """The oracle's result of case `name`(*args), computed once."""
    c = {"fly": fly, "special": special}[name](*args)
    return _frozen(ho.triangulate(c["hm"], c["P"], c["flip"], c["plane"], c["X0"], IMAGE_SHAPE, half, levels, floor))


def comparable(ref):
    """[n, J] bool: the oracle's gap exceeds GAP at every level."""
    return (ref["gap"] > GAP).all(axis=2)


def probe_points(c, M=24, seed=0):
    """pts [n, J, M, 3]: around the planted points -- inside the planes --, on plane edges (projections with a cell coordinate exactly 0 or
    H - 1 cannot be planted through a projection, so the edge rows and columns are reached by the views of special() that lie 0.6 cell
    inside an edge and points spread by a cell around them), far outside every plane, and the origin of the world."""
    rng = np.random.default_rng([seed, M])
    n, J = c["planted"].shape[:2]
    pts = c["planted"][:, :, None, :] + rng.normal(0.0, 0.15, (n, J, M, 3))
    pts[:, :, 0] = c["planted"]
    pts[:, :, 1] = c["planted"] + 50.0      # outside every plane
    pts[:, :, 2] = 0.0
    pts[:, :, 3] = c["planted"] + rng.normal(0.0, 1.0, (n, J, 3))
    return np.ascontiguousarray(pts)
