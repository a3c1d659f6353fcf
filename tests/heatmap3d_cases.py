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


# ---- the sweep (tests/test_gpu_heatmap3d_sweep.py, certified on the host by tests/test_heatmap3d_cases_host.py) -----------------------
def exact_cameras(H, W, V=2, behind=()):
    """(P [V, 3, 4], flip [V], image_shape) of ortho()'s cameras for planes [H, W] with cells of 4 rows by 8 columns of pixels, both powers
    of two and unequal: an even view has column = x + v / 8 and row = y, an odd one (flipped) column = W - (x + (v - 1) / 8) and row = z,
    all with w = 1 (-1 for the views in `behind`).  Every cell coordinate is the point's own coordinate to the bit, so windows and taps
    can be predicted by hand; the eighths tell apart views beyond the first two."""
    P = np.zeros((V, 3, 4))
    for v in range(V):
        P[v, 0, 0], P[v, 0, 3], P[v, 1, 1 + v % 2], P[v, 2, 3] = 8.0, 8.0 * (v // 2) / 8.0, 4.0, 1.0
        if v in behind:
            P[v] = -P[v]
    return P, (np.arange(V) % 2).astype(np.uint8), (8 * W, 4 * H)


def planted_maps(P, flip, plane, X, image_shape, C, H, W, sigma=1.0, reach=12):
    """hm [n, V, C, H, W] float32 of zeros with a Gaussian blob of deviation `sigma` cells added at the projection of X [n, J, 3] in the
    plane of every view of every joint, computed within `reach` cells of it (beyond 12 deviations float32 holds 0 anyway)."""
    n, J = X.shape[:2]
    cell = ho.cell_size(image_shape, H, W)
    hm = np.zeros((n, len(P), C, H, W), dtype=np.float32)
    for v in range(len(P)):
        for j in range(J):
            if plane[v, j] < 0:
                continue
            row_px, col_px, _ = ho.project(P[v], X[:, j])
            r, c = ho.to_cells(row_px, col_px, bool(flip[v]), cell, W)
            for t in range(n):
                if not (np.isfinite(r[t]) and np.isfinite(c[t]) and -reach < r[t] < H + reach and -reach < c[t] < W + reach):
                    continue
                r0, r1, c0, c1 = max(int(r[t]) - reach, 0), min(int(r[t]) + reach, H), max(int(c[t]) - reach, 0), min(int(c[t]) + reach, W)
                rr, cc = np.arange(r0, r1, dtype=np.float64)[:, None], np.arange(c0, c1, dtype=np.float64)[None, :]
                hm[t, v, plane[v, j], r0:r1, c0:c1] += np.exp(-0.5 * (((rr - r[t]) / sigma) ** 2 + ((cc - c[t]) / sigma) ** 2))
    return hm


def _case(hm, P, flip, plane, X0, image_shape, half, levels, floor=FLOOR, **more):
    return _frozen(dict(hm=hm, P=np.ascontiguousarray(P, dtype=np.float64), flip=np.asarray(flip, dtype=np.uint8),
                        plane=np.ascontiguousarray(plane, dtype=np.int32), X0=np.ascontiguousarray(X0, dtype=np.float64),
                        image_shape=tuple(image_shape), half=half, levels=levels, floor=floor, **more))


def _exact(H, W, X0, offsets, plane, C, half, levels, V=2, sigma=1.0, behind=()):
    P, flip, shape = exact_cameras(H, W, V, behind)
    X0 = np.array(X0, dtype=np.float64)
    planted = X0 + np.array(offsets, dtype=np.float64)
    plane = np.array(plane, dtype=np.int32)
    return _case(planted_maps(P, flip, plane, planted, shape, C, H, W, sigma), P, flip, plane, X0, shape, half, levels, planted=planted)


def _golden_case(H, W, views, flips, J, half=HALF, levels=LEVELS, seed=0, change=None):
    """n = 2 golden frames, the first J joints, C = J planes that every view numbers differently; `change(P, X0)` edits the cameras."""
    P7, pose = golden()
    P = np.ascontiguousarray(P7[list(views)])
    X0 = np.ascontiguousarray(pose[:2, :J])
    if change is not None:
        change(P, X0)
    planted = X0 + np.random.default_rng([11, seed, H, W]).normal(0.0, PLANT_MM, X0.shape)
    plane = np.array([[(v + j) % J for j in range(J)] for v in range(len(views))], dtype=np.int32)
    flip = np.array(flips, dtype=np.uint8)
    with np.errstate(all="ignore"):
        hm = planted_maps(P, flip, plane, planted, IMAGE_SHAPE, J, H, W)
    return _case(hm, P, flip, plane, X0, IMAGE_SHAPE, half, levels, planted=planted)


# one asymmetric patch per view: with the same patch in both, two points that swap their fractions between the views swap the views' terms
# and tie to the bit by the commutativity of the sum -- an exact tie of level 1 that nothing here constructs on purpose
TIE_PATCH = np.array([[[0.11, 0.07, 0.13, 0.05], [0.09, 0.93, 0.71, 0.12], [0.06, 0.64, 0.83, 0.08], [0.10, 0.14, 0.04, 0.15]],
                      [[0.03, 0.16, 0.08, 0.12], [0.14, 0.58, 0.97, 0.06], [0.05, 0.88, 0.49, 0.17], [0.13, 0.09, 0.11, 0.02]]], dtype=np.float32)
# a lane's own pair (i, i + 256); the lower index in the higher lane; four steps apart along z; and seven pairs (a, b) that meet at the
# steps o = 1, 2, 4 .. 64 of a halving tree over 256 lanes with b, the higher index, already in the receiving lane: a tree that keeps
# the receiver's point on equal scores -- the lower lane, not the lower index -- returns b.  (The first two pairs meet with a in the
# receiving lane and cannot tell.  At o = 128 the receiver's index is the sender's + 128, two steps along x: their 4 x 4 taps overlap,
# so no pair of separate patches reaches that step; it runs the same line of the loop as the other seven.)
TIE_PAIRS = ((37, 293), (200, 300), (73, 77), (73, 78), (74, 332), (77, 169), (73, 113), (81, 353), (105, 329), (73, 393))
TIE_CENTRE, TIE_HALF = (12.0, 8.0, 8.0), 4.0


def _ties():
    """Joint k holds layout k of TIE_PAIRS: planes of zeros with the view's TIE_PATCH under the 16 taps of both points of the pair, in both views.  The
    step of level 0 is one cell and every grid point lies at a half cell, so both points read the same 16 float32 values with the same
    weights: the two scores are the same float64 operations on the same numbers."""
    H, W = 16, 32
    P, flip, shape = exact_cameras(H, W)
    K = len(TIE_PAIRS)
    plane = np.array([list(range(K)), list(range(K))], dtype=np.int32)
    hm = np.zeros((1, 2, K, H, W), dtype=np.float32)
    for k, pair in enumerate(TIE_PAIRS):
        for i in pair:
            x, y, z = (TIE_CENTRE[a] + ((i // 64, i // 8 % 8, i % 8)[a] - 3.5) * (2.0 * TIE_HALF / 8) for a in range(3))
            for v, (r, c) in enumerate(((y, x), (z, W - x))):
                r0, c0 = int(np.floor(r)) - 1, int(np.floor(c)) - 1
                hm[0, v, k, r0:r0 + 4, c0:c0 + 4] = TIE_PATCH[v]
    return _case(hm, P, flip, plane, np.tile(np.array(TIE_CENTRE), (1, K, 1)), shape, TIE_HALF, 2)


def tie_meeting(a, b, lanes=256):
    """(o, index) of two of a level's points in a halving tree over `lanes` lanes, lane i % lanes holding point i: the step o at which
    their scores are compared, and which of the two then sits in the receiving (lower) lane."""
    la, lb = a % lanes, b % lanes
    o = (la ^ lb) & -(la ^ lb)
    return o, (b if lb & o == 0 else a)


def _budget(W, behind=()):
    """Two joints whose reachable cubes cover both planes: X0 +- 1.25 x 32 passes every edge, so each window is its whole plane."""
    return _exact(32, W, [[(32.0, 16.0, 16.0), (31.0, 15.0, 17.0)]], [[(-10.7, -4.8, 3.1), (13.6, 5.7, -7.6)]], [[0, 1], [1, 0]], 2, 32.0, 3,
                  sigma=2.0, behind=behind)


def _cut_w(P, X0):
    # view 1's plane w = 0 is moved to 0.1 mm behind the first start point: it cuts that joint's cube (w changes by up to 0.7 mm over
    # the 0.5 mm the cube reaches) and lies before, inside or behind the other joints' cubes
    P[1, 2, 3] -= float(P[1, 2, :3] @ X0[0, 0] + P[1, 2, 3]) - 0.1


def _cut_inf(P, X0):
    # u = 1e308 (x + 1) + ... overflows for x > 0.8: corners of some cubes project to an infinite column while the start point does not
    P[1, 0, 0] = P[1, 0, 3] = 1e308


def _floor():
    """floor = 2^-10, a float32: planes of cells exactly at the floor, one float32 step above and one below it.  Joint 0: all three and a
    blob; joint 1: only cells at and below the floor (status 2); joint 2: at and below, and in each view a single cell one step above the
    floor beside the start point (searched)."""
    H, W = 16, 32
    f = np.float32(2.0 ** -10)
    up, down = np.nextafter(f, np.float32(1.0)), np.nextafter(f, np.float32(0.0))
    P, flip, shape = exact_cameras(H, W)
    plane = np.array([[0, 1, 2], [2, 0, 1]], dtype=np.int32)
    X0 = np.array([[(12.3, 8.2, 7.1), (20.6, 5.3, 9.4), (9.7, 10.1, 6.2)]])
    planted = X0 + np.array([[(0.41, -0.33, 0.27), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]])
    blobs = planted_maps(P, flip, plane, planted[:, :1], shape, 3, H, W)
    k = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5)
    three, two = np.array([f, up, down], dtype=np.float32)[k % 3], np.array([f, down], dtype=np.float32)[k % 2]
    hm = np.empty((1, 2, 3, H, W), dtype=np.float32)
    for v in range(2):
        hm[0, v, plane[v, 0]] = np.where(blobs[0, v, plane[v, 0]] > 2.0 * f, blobs[0, v, plane[v, 0]], three)
        hm[0, v, plane[v, 1]] = two
        hm[0, v, plane[v, 2]] = two
    x, y, z = X0[0, 2]
    hm[0, 0, plane[0, 2], int(y) + 1, int(x)] = up          # view 0: row y, column x
    hm[0, 1, plane[1, 2], int(z), int(W - x) + 1] = up      # view 1: row z, column W - x
    # one level: around a single cell 1.2e-7 above the floor the scores of a second level lie 5e-10 apart, under GAP
    return _case(hm, P, flip, plane, X0, shape, 1.0, 1, floor=float(f), planted=planted, values=(f, up, down))


def _rand(seed, lo, hi, shape):
    return np.random.default_rng([23, seed]).uniform(lo, hi, shape)


def _wide_views():
    J = 64
    X0 = _rand(1, 2.5, 4.5, (1, J, 3))
    return _exact(8, 8, X0, _rand(2, -0.3, 0.3, (1, J, 3)), [[(j + 5 * v) % J for j in range(J)] for v in range(8)], J, 1.0, 3, V=8)


def _many():
    J = 64
    X0 = _rand(3, 2.5, 4.5, (4, J, 3))
    return _exact(8, 8, X0, _rand(4, -0.3, 0.3, (4, J, 3)), [[j for j in range(J)], [(j + 7) % J for j in range(J)]], J, 1.0, 2)


MANY_REPEAT = 275   # the four frames of "many" 275 times: n = 1 100, 70 400 workgroups, past 65 535

SWEEP = {
    # shapes
    "4x4": lambda: _exact(4, 4, [[(1.6, 1.4, 1.7), (1.3, 1.8, 1.2)]], [[(0.21, -0.17, 0.13), (-0.19, 0.23, 0.11)]], [[0, 1], [1, 0]], 2, 1.0, 2),
    "5x7": lambda: _exact(5, 7, [[(3.4, 2.3, 1.6), (2.7, 1.7, 2.4)]], [[(0.31, -0.27, 0.23), (-0.29, 0.13, -0.21)]], [[0, 1], [1, 0]], 2, 1.5, 3),
    "16x32": lambda: _exact(16, 32, _rand(5, (6.0, 4.0, 4.0), (25.0, 11.0, 11.0), (2, 3, 3)), _rand(6, -0.6, 0.6, (2, 3, 3)),
                            [[0, 1, 2], [2, 0, 1]], 3, 2.0, 4),
    "96x24 golden": lambda: _golden_case(96, 24, (0, 1, 2), (0, 1, 0), 3),
    "1024x1024": lambda: _exact(1024, 1024, [[(1018.0, 1017.5, 1019.0), (5.5, 1019.0, 1017.0)]],
                                [[(0.3, 0.1, 0.2), (-0.1, 0.1, 0.3)]], [[0, 0], [0, 0]], 1, 2.0, 2),
    # wide
    "C 1024": lambda: _exact(4, 4, [[(1.6, 1.4, 1.7), (1.3, 1.8, 1.2)]], [[(0.21, -0.17, 0.13), (-0.19, 0.23, 0.11)]],
                             [[1023, 0], [0, 1023]], 1024, 1.0, 2),
    "J 64, V 8": _wide_views,
    "J 1": lambda: _exact(8, 8, [[(3.3, 3.6, 4.2)]], [[(0.23, -0.31, 0.17)]], [[0], [0]], 1, 1.0, 3),
    "V 1": lambda: _exact(8, 8, _rand(7, 2.5, 4.5, (2, 3, 3)), np.zeros((2, 3, 3)), [[0, 1, 2]], 3, 1.0, 2, V=1),
    # ties, budget, cut, floor, many
    "ties": _ties,
    "budget 4096": lambda: _budget(64),
    "budget 4160": lambda: _budget(65),
    "budget behind": lambda: _budget(64, behind=(1,)),
    "cut w": lambda: _golden_case(16, 32, (0, 1, 2), (0, 1, 0), 3, change=_cut_w),
    "cut inf": lambda: _golden_case(16, 32, (0, 1, 2), (0, 1, 0), 6, change=_cut_inf),
    "floor": _floor,
    "many": _many,
}
FAMILIES = {"shapes": ("4x4", "5x7", "16x32", "96x24 golden", "1024x1024"), "wide": ("C 1024", "J 64, V 8", "J 1", "V 1"), "ties": ("ties",),
            "budget": ("budget 4096", "budget 4160", "budget behind"), "cut": ("cut w", "cut inf"), "floor": ("floor",), "many": ("many",)}
NONE_LEFT_OUT = FAMILIES["ties"] + FAMILIES["budget"] + FAMILIES["cut"] + FAMILIES["floor"]
ROUTES = ("fly", "special 8") + FAMILIES["budget"] + FAMILIES["cut"]   # the cases whose route is compared with the window model


@functools.lru_cache(maxsize=None)
def sweep(name):
    """Case `name`: dict of hm, P, flip, plane, X0, image_shape, half, levels, floor (and planted where blobs were planted)."""
    if name in ("fly", "special 8"):
        return _frozen(dict(fly(2) if name == "fly" else special(8), image_shape=IMAGE_SHAPE, half=HALF, levels=LEVELS, floor=FLOOR))
    return SWEEP[name]()


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    c = sweep(name)
    return _frozen(ho.triangulate(c["hm"], c["P"], c["flip"], c["plane"], c["X0"], c["image_shape"], c["half"], c["levels"], c["floor"]))


@functools.lru_cache(maxsize=None)
def sweep_windows(name):
    """(used [n, J], win [n, J, V, 4]) of the oracle's window model."""
    c = sweep(name)
    used, win = ho.windows(c["P"], c["flip"], c["plane"], c["X0"], c["image_shape"], *c["hm"].shape[3:], c["half"])
    used.setflags(write=False), win.setflags(write=False)
    return used, win


def level_points(c, ref, t, j, level):
    """(pts [512, 3], score [512]) of level `level` of the oracle's search of (t, j), which follows ref's choices."""
    centre, h = c["X0"][t, j].copy(), float(c["half"])
    for lv in range(level):
        step = 2.0 * h / ho.GRID
        centre, h = ho._grid_points(centre, step)[ref["choice"][t, j, lv]].copy(), step
    pts = ho._grid_points(centre, 2.0 * h / ho.GRID)
    logs = ho.Logs(c["hm"], c["floor"])
    cell = ho.cell_size(c["image_shape"], *c["hm"].shape[3:])
    s = np.zeros(len(pts))
    for v in range(len(c["P"])):
        if c["plane"][v, j] >= 0:
            s = s + ho.view_term(logs(t, v, int(c["plane"][v, j])), c["P"][v], bool(c["flip"][v]), pts, cell, logs.log_floor)
    return pts, s


def tied_by_construction(c, ref, t, j, level):
    """Whether the points of the level that share the best score are the same computation: in every view of the joint either none of them
    is informed, or all are, with the same bits of (f_r, f_c) and the same 16 float32 values under the taps in the same order."""
    pts, s = level_points(c, ref, t, j, level)
    tied = np.nonzero(s == s.max())[0]
    if len(tied) != ref["ties"][t, j, level] or tied[0] != ref["choice"][t, j, level]:
        return False
    cell = ho.cell_size(c["image_shape"], *c["hm"].shape[3:])
    for v in range(len(c["P"])):
        if c["plane"][v, j] < 0:
            continue
        ok, f, cells = ho.taps(c["hm"][t, v, c["plane"][v, j]], c["P"][v], bool(c["flip"][v]), pts[tied], cell)
        if ok.any() and not (ok.all() and all(f[i].tobytes() == f[0].tobytes() and cells[i].tobytes() == cells[0].tobytes() for i in range(len(tied)))):
            return False
    return True


def firm(c, ref):
    """[n, J] bool: every level of the search is firm -- its gap exceeds GAP, or its best score is shared by points that are tied by
    construction and stands more than GAP above every other score."""
    out = (ref["gap"] > GAP)
    for t, j, level in zip(*np.nonzero(~out & (ref["ties"] >= 2) & (ref["gap_next"] > GAP))):
        out[t, j, level] = tied_by_construction(c, ref, t, j, level)
    return out.all(axis=2)


def sweep_points(name, seed=0):
    """pts [n, J, M, 3] for the sampler: for the exact cameras every combination of coordinates on the plane's edges exactly, just outside
    them and inside, 64 uniform points and 16 around each of up to 8 planted points; for the golden cameras probe_points."""
    c = sweep(name)
    if "golden" in name or name.startswith("cut"):
        return probe_points(c)
    n, J = c["X0"].shape[:2]
    H, W = c["hm"].shape[3:]
    xs = (0.0, 0.5, 1.0, W / 2 + 0.25, W - 1.0, float(W), -0.001, W - 1 + 0.001)
    ys = (0.0, 0.75, H / 2 - 0.5, H - 1.0, -0.001, H - 1 + 0.001)
    grid = np.array([(x, y, z) for x in xs for y in ys for z in ys])
    pts = np.concatenate([grid, np.random.default_rng([seed, H, W]).uniform((0.0, 0.0, 0.0), (W - 1.0, H - 1.0, H - 1.0), (64, 3))])
    if "planted" in c:   # and on and around the blobs, which on the large planes the uniform points never meet
        near = c["planted"].reshape(-1, 3)[:8]
        pts = np.concatenate([pts, near, (near[:, None, :] + np.random.default_rng([seed, 1, H, W]).normal(0.0, 1.5, (len(near), 16, 3))).reshape(-1, 3)])
    return np.ascontiguousarray(np.broadcast_to(pts, (n, J, *pts.shape)))


def point_bar(c):
    """POINT_BAR of tests/test_gpu_heatmap3d.py for this case's coordinates: a level adds one product and one sum to each coordinate of
    the centre, two roundings of 2^-53 relative to the coordinate's magnitude M, and the shift one more; 2 levels M 2^-53 with the two
    orders of margin of that file, and never under its 1e-12 (which is this formula at 6 levels and the 4 mm of the golden pose: 5e-13)."""
    M = float(np.nanmax(np.abs(np.where(np.isfinite(c["X0"]), c["X0"], 0.0)))) + 2.0 * c["half"]
    return max(1e-12, 100.0 * 2.0 * c["levels"] * M * 2.0 ** -53)


def score_bar(c):
    """SCORE_BAR of tests/test_gpu_heatmap3d.py for this case: its largest term is a cell coordinate that differs by one rounding, times
    the slope of at most |log floor| = 7 per cell.  There the rounding was put at 1e-13 cells; a coordinate of M cells rounds by
    M 2^-53 (1.1e-13 at 1 024).  Two orders above that, and never under that file's 1e-10."""
    M = float(max(c["hm"].shape[3:]))
    return max(1e-10, 100.0 * 7.0 * M * 2.0 ** -53)


FIELDS = ("points3d", "score", "status", "views", "shift", "choice", "counts")


def compare(name, got, path, ref, X0, ok, point_bar, score_bar, what="under the gap of 1e-09"):
    """What every search test asserts of a device result `got` (dict of numpy arrays by FIELDS) and its `path` against the oracle's `ref`:
    views and the bookkeeping exactly; status, choice and counts exactly and points, shift and score within the bars on the searches `ok`
    [n, J] holds; at most MAX_SKIPPED of the searches outside `ok`."""
    searched = ref["status"] % 2 == 1
    skipped = int((searched & ~ok).sum())
    print(f"{name}: {int(searched.sum())} searched, {skipped} {what} (smallest gap {ref['gap'].min():.2e}), statuses "
          f"{np.bincount(ref['status'].ravel(), minlength=4).tolist()}, |score| {np.nanmax(np.abs(got['score'] - ref['score']), initial=0.0):.2e}")
    assert skipped <= MAX_SKIPPED * ref["status"].size
    assert got["status"].dtype == np.int8 and got["views"].dtype == np.int32 and got["choice"].dtype == np.int32 and got["counts"].dtype == np.int64
    assert np.array_equal(got["views"], ref["views"])
    assert np.array_equal(got["status"][ok], ref["status"][ok]) and np.array_equal(got["choice"][ok], ref["choice"][ok])
    assert np.array_equal(got["counts"], np.stack([(got["status"] == k).sum(axis=0) for k in range(4)], axis=1))
    if not skipped:
        assert np.array_equal(got["counts"], ref["counts"])
    moved = ok & searched
    assert np.abs(got["points3d"][moved] - ref["points"][moved]).max(initial=0.0) <= point_bar
    assert np.abs(got["shift"][moved] - ref["shift"][moved]).max(initial=0.0) <= point_bar
    assert np.abs(got["score"][moved] - ref["score"][moved]).max(initial=0.0) <= score_bar
    kept = ~searched
    assert got["points3d"][kept].tobytes() == X0[kept].tobytes() and not got["shift"][kept].any()
    assert np.array_equal(np.isnan(got["score"]), ref["status"] == 0)
    two = ref["status"] == 2
    assert np.abs(got["score"][two] - ref["score"][two]).max(initial=0.0) <= score_bar and (got["choice"][kept] == -1).all()
    assert np.array_equal(path == 0, ref["status"] == 0) and np.isin(path, (0, 1, 2)).all()
    return path
