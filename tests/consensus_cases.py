"""Seeded inputs for the consensus triangulation (csrc/consensus.hip): the eight-camera rig and the detections of
tests/pose_chain_cases.py (exact projections + N(0, 0.5 px)) with planted outliers.  Host numpy only.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import pose_chain_cases as pc

OUTLIER_PX = 60.0
TAU = 5.0
# (views, planted outliers): every layout with at least three clean views, where the model must return exactly the clean set
CLEAN_LAYOUTS = ((8, 1), (8, 2), (8, 3), (5, 1), (4, 1))
AMBIGUOUS_LAYOUT = (3, 1)      # two clean views: the wrong detection pairs with a clean one whenever it lies near an epipolar line
AMBIGUOUS_RECOVERED = 296      # of 300, what the oracle gives on these seeds (tests/test_consensus_host.py asserts it is that, and no more)
# The DLT of a candidate is compared with the SVD oracle (bar pose_chain_cases.TRI_BAR) on the CLEAN detections, all 247 subsets of the
# eight cameras: there the eigen-decomposition of the normal matrix agrees with the SVD within TRI_CONDITION at every size
# (tests/test_consensus_host.py).  A pair that holds a planted outlier is two rays that miss each other by far and is ill-conditioned
# (worst |eigh - SVD| 3.6e-9 over the pairs of planted(8, 1)): on the planted cases the choice is compared teacher-forced instead.
# The launches where the packing of points into passes matters are compared with the SVD too, on their clean variants
# (outliers=False), which meet the same condition.


def packed_clean_cases():
    """[(name, P, px)]: the clean variants of the launches whose points differ in their number of views."""
    out = [("staircase", rig(), staircase(outliers=False)),
           ("staircase [9, 3]", rig(), np.ascontiguousarray(staircase(outliers=False).reshape(8, 9, 3, 2))),
           ("fly layout", rig(7), fly_layout(outliers=False)[0])]
    return out + [(f"mixed {ncam} x {T} x {J}", rig(ncam), mixed(ncam, T, J, outliers=False)) for ncam, T, J in ((2, 3, 64), (3, 257, 1), (7, 5, 13))]


def rig(ncam=8):
    return np.ascontiguousarray(pc.rig()[0][:ncam])


@functools.lru_cache(maxsize=None)
def planted(views, outliers, seed=0, npoints=pc.TRI_POINTS):
    """(px [8, npoints, 1, 2], clean [npoints] bitmask): the first `views` cameras see every point, and `outliers` of them, drawn per
    point, are moved by OUTLIER_PX in a random direction.  Read only."""
    px = pc.detections(pc.TRI_SEED, npoints)[0].copy()
    px[views:] = 0.0
    rng = np.random.default_rng(1000 * views + 10 * outliers + seed)
    clean = np.full(npoints, (1 << views) - 1, dtype=np.int64)
    for i in range(npoints):
        for c in rng.choice(views, size=outliers, replace=False):
            a = rng.uniform(0.0, 2.0 * np.pi)
            px[c, i, 0] += OUTLIER_PX * np.array([np.sin(a), np.cos(a)])
            clean[i] &= ~(1 << int(c))
    assert (px[:views] != 0.0).all()
    px.setflags(write=False)
    clean.setflags(write=False)
    return px, clean


def shaped(px, ncam, T, J):
    """The first T J points of px [8, n, 1, 2] as [ncam, T, J, 2]."""
    return np.ascontiguousarray(px[:ncam, :T * J, 0].reshape(ncam, T, J, 2))


def mixed(ncam, T, J, seed=0, outliers=True):
    """[ncam, T, J, 2]: one planted outlier in a third of the points (none with outliers=False), one camera hidden in another third, the
    rest clean."""
    px = pc.detections(pc.TRI_SEED + 1 + seed, T * J)[0][:ncam, :, 0].copy()
    rng = np.random.default_rng(77 + seed)
    for i in range(T * J):
        c = int(rng.integers(ncam))
        if i % 3 == 0 and outliers:
            a = rng.uniform(0.0, 2.0 * np.pi)
            px[c, i] += OUTLIER_PX * np.array([np.sin(a), np.cos(a)])
        elif i % 3 == 1:
            px[c, i] = 0.0
    return np.ascontiguousarray(px.reshape(ncam, T, J, 2))


def staircase(npoints=27, outliers=True):
    """[8, npoints, 1, 2]: consecutive points see 0, 1, 2, ... 8 views in turn (point i: the cameras (i + k) mod 8, k < i mod 9), every
    third point with one planted outlier among its views (none with outliers=False: the clean detections)."""
    px = pc.detections(pc.TRI_SEED + 5, npoints)[0].copy()
    rng = np.random.default_rng(5)
    for i in range(npoints):
        seen = [(i + k) % 8 for k in range(i % 9)]
        for c in range(8):
            if c not in seen:
                px[c, i] = 0.0
        if outliers and i % 3 == 0 and seen:
            px[seen[int(rng.integers(len(seen)))], i, 0] += (OUTLIER_PX, -OUTLIER_PX)
    return px


def fly_layout(T=40, seed=0, outliers=True):
    """[7, T, 38, 2]: the visibility of config.camera_see_joint on the first seven cameras of the rig, an outlier planted in one view of
    every fifth point (none with outliers=False: the clean detections)."""
    from deepfly3d_amd.config import camera_see_joint

    px = pc.detections(pc.TRI_SEED + 9 + seed, T * 38)[0][:7, :, 0].copy().reshape(7, T, 38, 2)
    see = np.array([[camera_see_joint(c, j) for j in range(38)] for c in range(7)])
    px[~see[:, None, :].repeat(T, axis=1)] = 0.0
    rng = np.random.default_rng(9 + seed)
    for i in range(0, T * 38 if outliers else 0, 5):
        t, j = divmod(i, 38)
        seen = np.nonzero(see[:, j])[0]
        if seen.size:
            a = rng.uniform(0.0, 2.0 * np.pi)
            px[seen[int(rng.integers(seen.size))], t, j] += OUTLIER_PX * np.array([np.sin(a), np.cos(a)])
    return np.ascontiguousarray(px), see


def special(seed=0):
    """(P [8, 3, 4], px [8, 24, 1, 2]): camera 2's matrix negated, so every point lies behind it (w < 0: the DLT does not notice, the
    error does); points 0 .. 7 see all cameras, 8 .. 11 cameras (2, 5) only, 12 .. 15 cameras (1, 2, 5).  Points 16 .. 23 see five
    cameras and carry a NaN or an infinity in one coordinate of one or two of them."""
    P = rig().copy()
    P[2] = -P[2]
    px = pc.detections(pc.TRI_SEED + 3 + seed, 24)[0].copy()
    for i in range(8, 12):
        px[[0, 1, 3, 4, 6, 7], i] = 0.0
    for i in range(12, 16):
        px[[0, 3, 4, 6, 7], i] = 0.0
    px[5:, 16:] = 0.0
    for k, i in enumerate(range(16, 24)):
        bad = (np.nan, np.inf, -np.inf, np.nan)[k % 4]
        px[k % 2, i, 0, k % 2] = bad        # camera 0 or 1 is the negated one's neighbour: cameras 3 and 4 stay clean
        if k >= 4:
            px[3, i, 0, 1] = bad
    return P, px
