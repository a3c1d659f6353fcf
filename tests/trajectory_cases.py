"""Seeded inputs for the trajectory triangulation (csrc/trajectory.hip): points on planted smooth trajectories in
front of the rig of tests/pose_chain_cases.py, projected exactly and snapped to the 7.5 px cells of a heat-map.  Host numpy only.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import consensus_cases as cc
import consensus_oracle as co
import pose_chain_cases as pc

CELL = 7.5            # pixels per heat-map cell: a detection is the centre of its cell
OUTLIER_PX = 60.0
FPS = 100.0
LAMBDA, HUBER = 1e3, 10.0      # config's defaults, spelled out: the value tests are about these
GAP_STARTS, GAP_LEN = (50, 120, 190, 260, 330), 8
OUTLIER_EVERY = 10
# the cap tests/test_trajectory_host.py puts on the share of clean views of clean frames that end below weight 1: the oracle gives 0 of
# 720 in outliers(2) and 0 of 1 080 in outliers(3) at the defaults, so 1 % leaves room for a handful of views near
# the Huber threshold and none for a fit that misses the trajectory (15.8 % at lambda = 1e5)
CLEAN_DOWNWEIGHTED_CAP = 0.01


def rig(ncam=7):
    return cc.rig(ncam)


def sinusoid(T, J=1, hz=5.0, amp=1.0, seed=0):
    """X [T, J, 3] mm: joint j rests at the rig's centre plus N(0, 1) and swings by amp sin(2 pi hz t / FPS + phase_j) along a random
    unit direction, on top of a drift of 0.5 mm over the recording along another."""
    rng = np.random.default_rng([41, seed, J])
    rest = pc.rig()[1] + rng.normal(0.0, 1.0, size=(J, 3))
    swing, drift = rng.normal(size=(2, J, 3))
    swing /= np.linalg.norm(swing, axis=1, keepdims=True)
    drift /= np.linalg.norm(drift, axis=1, keepdims=True)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=J)
    t = np.arange(T, dtype=np.float64)
    return (rest[None] + amp * np.sin(2.0 * np.pi * hz * t[:, None] / FPS + phase[None])[..., None] * swing[None]
            + (0.5 * t / max(T - 1, 1))[:, None, None] * drift[None])


def project(P, X):
    """px [ncam, T, J, 2] (row, col), exact."""
    Xh = np.concatenate([X, np.ones(X.shape[:-1] + (1,))], axis=-1)
    uvw = np.einsum("cab,tjb->ctja", P, Xh)
    assert (uvw[..., 2] > 0.0).all()
    return np.stack([uvw[..., 1] / uvw[..., 2], uvw[..., 0] / uvw[..., 2]], axis=-1)


def quantise(px):
    q = (np.floor(px / CELL) + 0.5) * CELL
    assert (q != 0.0).all()
    return q


def dlt(P, px):
    """The plain triangulation the fit starts from: consensus_oracle.dlt (SVD), 0 where fewer than two views."""
    return co.dlt(P, px)


def _detections(T, J, cams, seed, hz=5.0):
    P = rig()
    X = sinusoid(T, J, hz=hz, seed=seed)
    px = quantise(project(P, X))
    hidden = [c for c in range(P.shape[0]) if c not in cams]
    px[hidden] = 0.0
    return P, px, X


@functools.lru_cache(maxsize=None)
def clean(nviews, T=400, J=1, seed=0, hz=5.0):
    """(P [7, 3, 4], px [7, T, J, 2], X_true [T, J, 3]): the first nviews cameras see every frame.  Read only."""
    out = _detections(T, J, range(nviews), seed, hz)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def one_view_gaps(T=400, J=1, seed=0, starts=GAP_STARTS):
    """(P, px, X_true, gap [T] bool): three views, but camera 0 alone in the GAP_LEN frames from each of `starts`.  Read only."""
    P, px, X = _detections(T, J, range(3), seed)
    gap = np.zeros(T, bool)
    for s in starts:
        gap[s : s + GAP_LEN] = True
    px[1:3, gap] = 0.0
    out = (P, px, X, gap)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def outliers(nviews, T=400, J=1, seed=0):
    """(P, px, X_true, planted [7, T, J] bool): one view of every OUTLIER_EVERY-th frame (from frame 5) moved by OUTLIER_PX in a random
    direction, then snapped to its cell.  Read only."""
    P, px, X = _detections(T, J, range(nviews), seed)
    exact = project(P, X)
    planted = np.zeros(px.shape[:3], bool)
    rng = np.random.default_rng([43, nviews, seed])
    for t in range(5, T, OUTLIER_EVERY):
        for j in range(J):
            c, a = int(rng.integers(nviews)), rng.uniform(0.0, 2.0 * np.pi)
            px[c, t, j] = quantise(exact[c, t, j] + OUTLIER_PX * np.array([np.sin(a), np.cos(a)]))
            planted[c, t, j] = True
    out = (P, px, X, planted)
    for a in out:
        a.setflags(write=False)
    return out


def fly(T, seed=0):
    """(P, px [7, T, 38, 2], X_true): the 38 joints under config.camera_see_joint's visibility, an outlier in one view of every 19th
    point, camera-1 detections of joint 3 hidden in frames 10 .. 14 and every view of joint 7 hidden in frames 20 .. 22."""
    from deepfly3d_amd.config import camera_see_joint

    P = rig()
    X = sinusoid(T, 38, seed=seed + 7)
    exact = project(P, X)
    px = quantise(exact)
    see = np.array([[camera_see_joint(c, j) for j in range(38)] for c in range(7)])
    px[~np.broadcast_to(see[:, None, :], px.shape[:3])] = 0.0
    rng = np.random.default_rng([47, T, seed])
    for i in range(0, T * 38, 19):
        t, j = divmod(i, 38)
        seen = np.nonzero(see[:, j])[0]
        if seen.size:
            c, a = int(seen[int(rng.integers(seen.size))]), rng.uniform(0.0, 2.0 * np.pi)
            px[c, t, j] = quantise(exact[c, t, j] + OUTLIER_PX * np.array([np.sin(a), np.cos(a)]))
    px[1, 10:15, 3] = 0.0
    px[:, 20:23, 7] = 0.0
    return P, np.ascontiguousarray(px), X


def rms(a, b, rows=None):
    d = np.linalg.norm(np.asarray(a, np.float64) - b, axis=-1)
    return float(np.sqrt(np.mean((d if rows is None else d[rows]) ** 2)))


# ---- the banded solve ------------------------------------------------------------------------------------------------------------------
SOLVE_LAMBDAS = (0.0, 1.0, 1e4, 1e8)
SOLVE_MU = 1e-3
SOLVE_BLOCKS = (3, 7, 64, 1 << 20)      # the range's minimum, an odd size, the size of a wave, the serial factorisation


def solve_lengths(B):
    """The chain lengths a block size is tested at."""
    return sorted({T for T in (3, 4, 5, B - 1, B, B + 1, 2 * B + 1, 257) if 3 <= T <= 257})


def segment_table(T, J, B):
    """[T, J] int8.  Chain j takes pattern j % 4 (a lone chain: pattern 3): 0 every frame active; 1 the first and the last frame are
    not; 2 a break on a separator (frame Bc - 2) and on the frame after the first block; 3 a break inside the first block, one on the
    last frame of the second block, and the first frame.  A frame is switched off only where the chain is long enough to hold it."""
    Bc = min(B, max(T, 3))
    seg = np.ones((T, J), np.int8)
    for j in range(J):
        off = {0: (), 1: (0, T - 1), 2: (Bc - 2, Bc), 3: (0, Bc // 2, 2 * Bc - 1)}[3 if J == 1 else j % 4]
        for t in off:
            if 0 <= t < T and T >= 6:
                seg[t, j] = 0
    return seg


@functools.lru_cache(maxsize=None)
def solve_terms(T, J):
    """(H [T, J, 6], g [T, J, 3], X [T, J, 3]) of a real linearisation: the fly layout's detections (J = 38) or the three-view outlier
    case (J = 1) at the plain triangulation, HUBER px.  Read only."""
    import trajectory_oracle as to

    P, px = (fly(T)[:2] if J == 38 else outliers(3, T, J)[:2])
    X = dlt(P, px)
    H, g, _, _, _ = to.linearize(P, px, X, HUBER)
    for a in (H, g, X):
        a.setflags(write=False)
    return H, g, X


def solve_system(T, J, B, lam):
    """(AB, b, seg, g_whole): the system the device is given, in the oracle's band form."""
    import trajectory_oracle as to

    H, g, X = solve_terms(T, J)
    seg = segment_table(T, J, B)
    active = seg != 0
    c = to.centres(active)
    lam = np.full(J, lam)
    G = g + lam[None, :, None] * to.smoothness(X, c)[1]
    AB, b = to.system(H, G, c, active, lam, np.full(J, SOLVE_MU))
    return AB, b, seg, G


# ---- the whole fit ---------------------------------------------------------------------------------------------------------------------
FIT_LENGTHS = (40, 257)
FIT_BLOCKS = (3, 16, 64, 1 << 20)
FIT_CASES = ("gaps", "outliers2", "outliers3", "clean2", "clean3", "fly")


def fit_case(name, T):
    """(P, px) of a whole-fit case at T frames."""
    if name == "gaps":
        return one_view_gaps(T, 2, starts=(10, 24) if T < 100 else (50, 120, 190))[:2]
    if name.startswith("outliers"):
        return outliers(int(name[-1]), T, 2)[:2]
    if name.startswith("clean"):
        return clean(int(name[-1]), T, 2)[:2]
    return fly(T)[:2]
