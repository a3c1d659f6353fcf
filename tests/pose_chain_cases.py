"""Seeded inputs for the sweep of the 3-D pose chain's kernels (csrc/geometry.hip, csrc/geometry_dev.h, csrc/pose3d.hip): re-layout,
DLT triangulation, exact medians, Procrustes, One-Euro.  tests/test_pose_chain_cases_host.py proves on the CPU, on the oracles alone,
what tests/test_gpu_pose_chain_sweep.py leans on; the latter runs the kernels.  Host numpy only.  TEST INFRASTRUCTURE ONLY.

Triangulation cases: the eight-camera rig of tests/ba_cases.py (cameras(8)), points N(0, 1 mm) round the rig centre, detections = exact
projections + N(0, 0.5 px) as (row, col) pixels, [8, n, 1, 2].  A camera subset is run as ncam = 8 with the other cameras' detections
zero ("not seen").

Bars (none is taken from a kernel):
  * triangulation, 1e-9 mm against oracle.geometry.triangulate_dlt (the bar of tests/test_gpu_geometry.py).  The kernel diagonalises the
    normal matrix A^T A / trace, so the condition is that an independent float64 statement of THAT method (triangulate_eigh below) agrees
    with the SVD oracle within 1e-10, a decade under the bar, on every case of the sweep, none excluded.  Measured worst |eigh - SVD| with
    TRI_SEED, TRI_POINTS points (tests/test_pose_chain_cases_host.py prints them):
        all 28 two-camera subsets    2.5e-11  (pair (1, 5))
        all 56 three-camera subsets  1.2e-13
        eight cameras                2.4e-14
  * Procrustes, 1e-10 against oracle.geometry.procrustes_separate (the bar of test_procrustes_long_sequence_against_oracle).  The
    condition is that the oracle's own spread under last-bit noise in its input (x (1 + 4 eps U(-1, 1))) stays below 1e-12 over all
    PROCRUSTES_DRAWS x 4 lengths x 2 templates = 400 draws.  Measured: 4.8e-13; the smallest s_min / s_max of a draw's
    fit is 4.6e-3, far from the kernel's rank cut of 1e-13.
  * everything else is bit-exact (numpy.array_equal).
"""
import functools
import itertools
import os

import numpy as np

import ba_cases as bc
from oracle import geometry as og

GOLDEN = bc.GOLDEN
EPS = np.finfo(np.float64).eps

# ---------------------------------------------------------------- re-layout ----------------------------------------------------------
ORDERINGS = tuple(itertools.permutations(range(7)))          # all 5040
RELAYOUT_EDGE_T = (1, 3, 7, 255, 256, 257)                   # 7 * T * 38 crosses multiples of the 256-thread block
BELOW_ONE = np.nextafter(np.float32(1.0), np.float32(0.0))   # 1 - 2^-24: un-flipped to 2^-24, the smallest non-zero column a left camera can give


def relayout_input(T, seed=0):
    """[7, T, 19, 2] float32 in [0, 1); every camera's first frame has 0.0, 1.0 and the float32 just below 1 as COLUMN of joints 0, 7, 18 (a
    leg joint, one more, the last stripe), its last frame has them in joints 16, 4, 11."""
    rng = np.random.default_rng(seed)
    p = rng.random((7, T, 19, 2)).astype(np.float32)    # rounded from float64: below 0.5 finer than 2^-24, so 1 - col is inexact in float32
    for t, joints in ((0, (0, 7, 18)), (T - 1, (16, 4, 11))):
        for j, v in zip(joints, (np.float32(0.0), np.float32(1.0), BELOW_ONE)):
            p[:, t, j, 1] = v
    return p


# ---------------------------------------------------------------- triangulation ------------------------------------------------------
TRI_SEED, TRI_POINTS = 11, 300
TRI_SUBSETS = tuple(s for k in (2, 3, 8) for s in itertools.combinations(range(8), k))   # 28 + 56 + 1
TRI_BAR, TRI_CONDITION = 1e-9, 1e-10


@functools.lru_cache(maxsize=None)
def rig():
    """P [8, 3, 4] of the eight-camera rig and its centre."""
    R, tvec, intr, centre = bc.cameras(8)
    return og.projection_matrices(R, tvec, intr), centre


@functools.lru_cache(maxsize=None)
def detections(seed=TRI_SEED, npoints=TRI_POINTS):
    """(px [8, npoints, 1, 2] (row, col) pixels, every camera seeing every point; X [npoints, 3] the true points).  Read only."""
    R, tvec, intr, centre = bc.cameras(8)
    rng = np.random.default_rng(seed)
    X = centre + rng.normal(0.0, 1.0, size=(npoints, 3))
    xy, depth = bc.project(R, tvec, intr, X)
    xy = xy + rng.normal(0.0, 0.5, size=xy.shape)
    assert (depth > 0.1).all() and (xy != 0).all()
    px = np.stack([xy[..., 1], xy[..., 0]], axis=-1)[:, :, None, :]
    px.setflags(write=False)
    return px, X


def only_cameras(px, cams):
    """px with the detections of every camera outside `cams` set to zero."""
    out = np.zeros_like(px)
    out[list(cams)] = px[list(cams)]
    return out


def triangulate_eigh(px, P):
    """The kernel's METHOD in plain float64 numpy, independent of its arithmetic: the eigenvector of the smallest eigenvalue of
    A^T A / trace(A^T A) by numpy.linalg.eigh, A as in oracle.geometry.triangulate_dlt.  [T, J, 3]; 0 where fewer than two views."""
    p = np.asarray(px, np.float64)
    vis = og.visibility(p)
    r0 = p[..., 1:2] * P[:, None, None, 2, :] - P[:, None, None, 0, :]
    r1 = p[..., 0:1] * P[:, None, None, 2, :] - P[:, None, None, 1, :]
    A = np.stack([r0, r1], axis=-2) * vis[..., None, None]
    M = np.einsum("ctjri,ctjrk->tjik", A, A)
    tr = np.trace(M, axis1=-2, axis2=-1)
    ok = vis.sum(axis=0) >= 2
    M = M / np.where(tr > 0, tr, 1.0)[..., None, None]
    v = np.linalg.eigh(M)[1][..., :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        X = v[..., :3] / v[..., 3:4]
    return np.where(ok[..., None], X, 0.0)


@functools.lru_cache(maxsize=None)
def tri_oracle(cams):
    """oracle.geometry.triangulate_dlt of the sweep's detections seen by `cams` only, [TRI_POINTS, 1, 3].  Read only."""
    ref = og.triangulate_dlt(only_cameras(detections()[0], cams), rig()[0])
    ref.setflags(write=False)
    return ref


def visibility_case():
    """px [8, 4, 1, 2] for the visibility rule: point 0 has exactly two views (cameras 0 and 1); point 1's only two "views" have one zero
    coordinate each; point 2 is seen by all but has -0.0 as camera 0's row and as camera 1's column; point 3 has one view."""
    px = detections()[0][:, :4].copy()
    px[2:, 0] = 0.0
    px[:, 1] = 0.0
    px[0, 1, 0, 0] = 5.0
    px[1, 1, 0, 1] = 7.0
    px[0, 2, 0, 0] = -0.0
    px[1, 2, 0, 1] = -0.0
    px[1:, 3] = 0.0
    return px


# ---------------------------------------------------------------- medians ------------------------------------------------------------
MED_LONG = 65536                       # csrc/pose3d.hip: columns at least this long take the multi-workgroup route when scratch is there
MED_LONG_WORK = 8 + 3 * 272            # 824 doubles = 8 + 3 * MED_SCRATCH_DOUBLES: the smallest pose_normalize work buffer that takes it
COLUMN_MEDIAN_N = (1, 2, 255, 256, 257, 65535, 65536, 65537)
# (T, J) of ops.pose_normalize: the route switch at J = 1, the first lengths past a multiple of the 4096 values one workgroup of the long
# route covers, the switch at 38 joints (1724 * 38 = 65512, 1725 * 38 = 65550), and one length above it at a small and a large J
NORMALIZE_SHAPES = ((65535, 1), (65536, 1), (65537, 1), (65536 + 4 * 4096 - 1, 1), (65536 + 4 * 4096 + 1, 1), (1724, 38), (1725, 38),
                    (13108, 5), (1025, 64))
COLUMN_KINDS = ("equal", "halves", "low_byte", "signed_zeros", "infs", "denormals", "sorted", "reversed", "ties")


def median_column(kind, n, seed=0):
    """One column of n doubles whose radix select goes a particular way."""
    rng = np.random.default_rng([seed, COLUMN_KINDS.index(kind), n])
    if kind == "equal":                    # one bin in every pass
        return np.full(n, -2.625)
    if kind == "halves":                   # two values, n // 2 of the larger: at even n the two middle ranks part in the FIRST pass (the sign bit)
        c = np.where(np.arange(n) < n // 2, 3.5, -1.25)
        return rng.permutation(c)
    if kind == "low_byte":                 # values that differ in their lowest mantissa byte only: the ranks part in the LAST pass
        bits = np.float64(1.7).view(np.uint64) & ~np.uint64(0xFF)
        return (bits | rng.integers(0, 256, size=n).astype(np.uint64)).view(np.float64)
    if kind == "signed_zeros":
        return rng.permutation(np.where(np.arange(n) % 2 == 0, -0.0, 0.0))
    if kind == "infs":                     # a few infinities of either sign, fewer than half: the median is finite
        c = rng.normal(0.0, 2.0, size=n)
        k = max(1, n // 8) if n > 3 else 0
        idx = rng.choice(n, size=k, replace=False)
        c[idx] = np.where(np.arange(k) % 3 == 0, -np.inf, np.inf)
        return c
    if kind == "denormals":
        return rng.integers(-(1 << 40), 1 << 40, size=n).astype(np.float64) * 5e-324
    if kind == "sorted":
        return np.cumsum(rng.random(n) + 0.001) - 0.3 * n      # strictly increasing, of both signs
    if kind == "reversed":
        return (np.cumsum(rng.random(n) + 0.001) - 0.3 * n)[::-1].copy()
    if kind == "ties":
        return np.round(rng.normal(0.0, 3.0, size=n), 1)
    raise ValueError(kind)


def median_runs(n, seed=0):
    """The nine column kinds as three [n, 3] blocks (one kind per axis)."""
    cols = [median_column(k, n, seed) for k in COLUMN_KINDS]
    return [np.stack(cols[i : i + 3], axis=1) for i in (0, 3, 6)]


# ---------------------------------------------------------------- Procrustes ---------------------------------------------------------
PROCRUSTES_BAR, PROCRUSTES_CONDITION = 1e-10, 1e-12
PROCRUSTES_T = (1, 2, 3, 15)
PROCRUSTES_DRAWS = 50                  # per length and template
PROCRUSTES_SWITCH_T = (3449, 3450)     # 3449 * 19 = 65531 < MED_LONG <= 65550 = 3450 * 19: the strided medians change route
SIDES = (slice(0, 19), slice(19, 38))
FIT_JOINTS = (0, 1, 5, 6, 10, 11)      # body-coxa and coxa-femur of the three legs, among a side's 19 joints
RANK_CUT = 1e-13                       # rigid_fit_kernel: a singular value below RANK_CUT * s_max is "weak"


@functools.lru_cache(maxsize=None)
def golden_pose():
    """The 15-frame triangulated pose of the golden recording, [15, 38, 3].  Read only."""
    p = np.load(os.path.join(GOLDEN, "golden_3d.npz"))["points3d_wo_procrustes"].astype(np.float64)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def templates():
    """name -> template pose [F, 38, 3]: the package's default and tests/golden/template.npz."""
    from deepfly3d_amd.config import load_procrustes_template

    return {"default": np.asarray(load_procrustes_template(), np.float64), "golden": np.load(os.path.join(GOLDEN, "template.npz"))["points3d"].astype(np.float64)}


def rigid_motion(rng, reflect):
    """(Q, scale, offset): a random orthogonal Q (det -1 if reflect), scale 10^U(-1, 1), offset N(0, 5)."""
    Q, Rr = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(Rr))
    if (np.linalg.det(Q) < 0) != bool(reflect):
        Q[:, 0] = -Q[:, 0]
    return Q, 10.0 ** rng.uniform(-1.0, 1.0), rng.normal(0.0, 5.0, size=3)


def moved_pose(T, draw):
    """The first T golden frames under the draw-th seeded rigid motion; every third draw is a reflection."""
    rng = np.random.default_rng([97, T, draw])
    Q, s, off = rigid_motion(rng, reflect=draw % 3 == 2)
    return s * (golden_pose()[:T] @ Q) + off


def long_pose(T):
    """T frames built like test_procrustes_long_sequence_against_oracle: the golden frames tiled, scaled, jittered and moved."""
    rng = np.random.default_rng(5)
    base = np.tile(golden_pose(), (T // 15 + 1, 1, 1))[:T]
    return base * 1.7 + rng.normal(0.0, 0.05, size=base.shape) + np.array([0.3, -1.0, 2.0])


def degenerate_pose(case, side):
    """The golden 15 frames with fit joints of `side` (0 or 1) lost, a lost joint being (0, 0, 0) as an untriangulated one is:
      "coplanar":  body-coxa and coxa-femur of legs 2 and 3 are zero in every frame -- the six median fit joints are three distinct points;
      "collinear": in addition leg 1's body-coxa is zero in 10 of the 15 frames -- two distinct points.
    Only the two FIT joints of legs 2 and 3 are zeroed: with the whole legs at zero eight of the twelve median segment lengths are 0, the
    median scale ratio is infinite and the side is NaN in the oracle and the kernel alike (`zero_legs_pose`, compared as such)."""
    p = golden_pose().copy()
    lo = 19 * side
    p[:, [lo + 5, lo + 6, lo + 10, lo + 11]] = 0.0
    if case == "collinear":
        p[np.arange(15) % 3 != 0, lo] = 0.0
    elif case != "coplanar":
        raise ValueError(case)
    return p


def zero_legs_pose(side):
    """The golden 15 frames with all ten joints of legs 2 and 3 of `side` at zero: an infinite scale, NaN on that side."""
    p = golden_pose().copy()
    p[:, 19 * side + 5 : 19 * side + 15] = 0.0
    return p


def oracle_procrustes(X, tmpl):
    """oracle.geometry.procrustes_separate, quiet about the infinite ratio of a zero-length segment."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return og.procrustes_separate(X, tmpl)


def zero_side_pose(side):
    """The golden 15 frames with every joint of `side` at zero (a side no camera pair saw): NaN on that side."""
    p = golden_pose().copy()
    p[:, SIDES[side]] = 0.0
    return p


def side_fit(pts_side, tmpl_side):
    """oracle.geometry._procrustes_side in pieces: scale s, centre m, the median fit joints of the template X and of the scaled, centred
    sequence Y [6, 3], the normalised G = X0^T Y0 whose SVD gives the rotation, and the oracle's (Tm, c)."""
    with np.errstate(all="ignore"):   # (a segment between two lost joints has length 0: an infinite ratio)
        s = np.median(np.median(og._bone_lengths(tmpl_side), axis=0) / np.median(og._bone_lengths(pts_side), axis=0))
        m = np.median(pts_side.reshape(-1, 3), axis=0)
        Y = np.median(((pts_side - m) * s)[:, list(FIT_JOINTS)], axis=0)
        X = np.median(tmpl_side[:, list(FIT_JOINTS)], axis=0)
        X0, Y0 = X - X.mean(0), Y - Y.mean(0)
        G = (X0 / np.sqrt((X0**2).sum())).T @ (Y0 / np.sqrt((Y0**2).sum()))
    Tm, c = og._rigid_fit(X, Y) if np.isfinite(G).all() else (None, None)   # (numpy's SVD raises on a non-finite matrix)
    return dict(s=s, m=m, X=X, Y=Y, G=G, Tm=Tm, c=c)


# ---------------------------------------------------------------- One-Euro -----------------------------------------------------------
ONEEURO_T = (1, 2, 3)
ONEEURO_NCH = (1, 63, 64, 65, 129)     # round the 64-thread block of oneeuro_kernel


def oneeuro_input(T, nch):
    return np.cumsum(np.random.default_rng([3, T, nch]).normal(0.0, 0.1, size=(T, nch)), axis=0)
