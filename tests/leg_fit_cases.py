"""Seeded hard inputs for the sweep of the constant-length leg fit's damped branch (csrc/leg_fit.hip): trials that
are rejected at a pivot or on cost, lambda climbing and coming back, legs that run out of iterations or stall, geometric ties and
thresholds, and one batch whose waves hold lanes that leave the loop at very different passes.  tests/test_leg_fit_cases_host.py
certifies on the CPU, on the float64 oracle alone, that every family does what it is there for; tests/test_gpu_leg_fit_sweep.py runs
the kernel on them.  Host numpy only.  TEST INFRASTRUCTURE ONLY.

A family is (X [T, 38, 3], lengths [6, 4], anchor [6, 3] or None, max_iter), in millimetre-sized coordinates; base_lengths() is the
golden recording's median lengths, FRAMES frames per seeded family.  families():
  noisy, noisy_free            synthetic_flies(noise = 0.5), anchored and not
  long, long_free, long_offset noise 0.3 fitted with 3 x the lengths; the last with the anchor moved by a few lengths
  short, short_free            noise 0.3 fitted with 0.2 x the lengths
  compressed, compressed_free  the noisy legs pulled to 0.05 of their size towards the anchor: the chain must fold
  limited_<m>                  8 frames of short at max_iter = m: 1, 2, 3, 7 and every count n at which one of its legs converges, and n - 1
  stalled, stalled_free        noisy with one leg's lengths x 1e160: that leg stalls on NaN pivots, the others converge
  edges                        ties of the tangent basis' axis choice (14 directions, -0.0 components), a straight reachable leg, a target
                               chain twice too long, antiparallel segments, a tip on the anchor, a start segment either side of TINY,
                               LAMBDA_MAX itself tried and accepted, a stall in finite arithmetic (EDGE_LEGS names the legs)
  tie_step                     one leg on which the lowest-index tie rule decides `small` (see _tie_sensitive_leg)
  milli, kilo, shifted         noisy x 1e-3, x 1e3, and + 1e6 mm without an anchor
  mixed, mixed_free            compressed, easy and noisy frames in turn with the stalled lengths table and missing legs: every run of
                               64 lanes g = 6 t + leg holds lanes that end at pass 0, at 3-8, at exactly 17 (stalled) and beyond 20
No seeded leg stalls in finite arithmetic (the host test asserts it); the constructed finite_stall leg of `edges` does.
`fit(name)` is the oracle's answer with every leg's trace, memoised per leg by its inputs' bits.

Bars of the GPU sweep (none is taken from the kernel).  MEASURED[name] = (legs whose (status, iters) differ between the oracle's two
arithmetic paths, basis_variant False and True; among the legs that agree, the largest point difference in mm per unit of scale and
the largest relative cost difference), recomputed by the host test, which fails if they drift.  The kernel is a third path of the same
kind, with contracted multiply-adds, so its bar is ten times the measured figure (the project's margin), and never below the existing
bar of tests/test_gpu_leg_fit.py; both times the coordinate scale (scale(): the binade of the family's largest coordinate, 1 for the
golden recording; leg_scale(): a leg's own where its coordinates lie beyond FAR):
    points   max(10 x measured, CONVERGED_BAR) x scale        cost   max(10 x measured, COST_RTOL)
"""
import collections
import functools
import os

import numpy as np

import leg_fit_oracle as lo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAMES = 24
SEED = 4                # of seeds 0..4 the first at which the oracle's two paths agree on every leg's (status, iters) in every family
STALLED_LEG = 4
HUGE = 1e160            # x the lengths of STALLED_LEG: len^2 overflows, 0 x inf and inf - inf make the first pivot NaN at every lambda
FLIP_CAP = 0.01         # kernel against oracle: the share of a family's fitted legs whose (status, iters) may differ
ORACLE_FLIP_CAP = 0.005   # the oracle's two paths against each other: the condition under which FLIP_CAP means something

Family = collections.namedtuple("Family", "X L A max_iter")
LEG_JOINTS = [j for leg in range(6) for j in lo.leg_joints(leg)]


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def base_lengths():
    X = np.load(os.path.join(GOLDEN, "golden_3d.npz"))["points3d_wo_procrustes"]
    return _frozen(lo.median_lengths(X))[0]


def stalled_lengths():
    L = base_lengths().copy()
    L[STALLED_LEG] *= HUGE
    return L


FAR = 1e9               # mm: coordinates beyond it belong to single constructed legs (lambda_max_tried, finite_stall) and scale their own bars
RIGID_COST = 1e-24      # mm^2 on coordinates of scale 1: below it a cost is that of an exact fit (tests/test_gpu_leg_fit.py)


def scale(X):
    """The binade of the largest finite coordinate up to FAR, halved: the factor on bars that were measured on the golden recording,
    whose largest coordinate is 3.9 mm (scale 1)."""
    a = np.abs(np.asarray(X, dtype=np.float64))
    return float(2.0 ** (np.floor(np.log2(a[np.isfinite(a) & (a <= FAR)].max())) - 1.0))


@functools.lru_cache(maxsize=None)
def _flies(noise, T=FRAMES):
    """synthetic_flies of the one seed: the same six body-coxa positions and the same rigid legs for every noise."""
    return _frozen(*lo.synthetic_flies(np.random.default_rng(SEED), T, base_lengths(), noise=noise))


def _compressed(X, A, factor=0.05):
    Y = X.copy()
    for leg in range(6):
        j = lo.leg_joints(leg)
        Y[:, j] = A[leg] + factor * (X[:, j] - A[leg])
    return Y


# ------------------------------------------------------------------------------------------------------------------ geometry edges
_STEP = 0.5   # a dyadic step: every sum and difference below is exact, so the ties are ties in the start directions' bits
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGONALS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


def _pose(rng, legs):
    """[38, 3]: legs {leg: P [5, 3]}; every other leg a mildly noisy synthetic one, the eight other joints noise."""
    X = _flies(0.02)[0][int(rng.integers(FRAMES))].copy()
    for leg, P in legs.items():
        X[lo.leg_joints(leg)] = P
    return X


def _chain_from(p0, segments):
    return np.concatenate([[p0], p0 + np.cumsum(np.asarray(segments, dtype=np.float64), axis=0)])


def _tie_poses():
    """Three poses whose 18 legs' 72 start segments run through the fourteen tie directions (six axes: two components tie at zero;
    eight diagonals: all three tie), consecutive segments never parallel; plus one pose whose first segments hold -0.0 components."""
    dirs = [np.array(d, dtype=np.float64) for d in AXES + DIAGONALS]
    poses, n = [], 0
    for f in range(3):
        legs = {}
        for leg in range(6):
            segs, prev = [], None
            while len(segs) < 4:
                d = dirs[n % 14]
                n += 1
                if prev is not None and abs(d @ prev) == (d @ d) ** 0.5 * (prev @ prev) ** 0.5:
                    continue
                segs.append(d * _STEP * (1 + len(segs) % 2))
                prev = d
            n += 4   # the next leg starts elsewhere in the list: no two legs run through the same four directions
            legs[leg] = _chain_from(np.array([-1.0, -2.0, -1.5]) + 0.25 * leg, segs)
        poses.append(_pose(np.random.default_rng(100 + f), legs))
    # -0.0: (-0.0) - (+0.0) = -0.0, so P0 holds +0.0 and P1 -0.0 in the components that are to tie as negative zeros
    legs = {}
    for leg, axis in enumerate([0, 1, 2, 0, 1, 2]):
        p0 = np.zeros(3)
        p0[axis] = -1.0 - 0.25 * leg
        s1 = np.array([-0.0, -0.0, -0.0])
        s1[axis] = 0.75
        P = _chain_from(p0, [s1, [0.5, 0.25, -0.5], [-0.25, 0.5, 0.5], [0.5, 0.5, 0.25]])
        P[1] = p0 + 0.0
        P[1][axis] = p0[axis] + 0.75
        for c in range(3):
            if c != axis:
                P[1][c] = -0.0
        legs[leg] = P
    poses.append(_pose(np.random.default_rng(103), legs))
    return poses


def _tie_sensitive_leg():
    """A leg one step of 0.85e-9 from its minimum whose first three start directions are exactly (1, 1, 1)/sqrt(3), all three
    components tied: a straight target chain whose first three joints lie RHO short of the chain's and whose tip 4 RHO beyond, so
    that the straight fit is the minimum, its cost is 19 RHO^2 and the first segment is the softest; the tip is then moved sideways
    by TIE_SENSITIVE_TIP.  With the axis of the lowest index the step's largest tangent coordinate is under TOL
    and the leg converges at once; with the axis of the highest index the same step has a coordinate above TOL (the two bases are
    turned by 120 degrees) and one more iteration follows.  The margins either side of TOL are 15 %, a million
    times the rounding of the step.  Found by a seeded search; the host test certifies both counts."""
    L = base_lengths()[TIE_SENSITIVE[1]]
    rng = np.random.default_rng(TIE_SENSITIVE_SEED)
    P = np.full((5, 3), -1.0)
    along = np.cumsum(L) + TIE_SENSITIVE_RHO * np.array([-1.0, -1.0, -1.0, 4.0])
    P[1:] += (along / np.sqrt(3.0))[:, None]   # the three components of every joint: the same bits
    P[4] = P[4] + TIE_SENSITIVE_TIP * lo._unit(rng.normal(size=3))
    return P


TIE_SENSITIVE = (0, 1)          # (frame, leg) in the "tie_step" family
TIE_SENSITIVE_RHO = 0.1
TIE_SENSITIVE_SEED = 15         # the first seed of a search over 0..299 with both margins at 15 % or more
TIE_SENSITIVE_TIP = 1.17355813640586e-08   # mm: scales the step to 0.85e-9


def _threshold_legs():
    """(not fitted, fitted): a start segment with |s_3|^2 / max |t_k|^2 = 0.5e-18 and 2e-18, a factor of two either side of TINY."""
    P = _flies(0.02)[0][3, lo.leg_joints(2)].copy()
    tmax = np.sqrt(((P[1:] - P[0]) ** 2).sum(axis=1).max())
    out = []
    for ratio in (0.5e-18, 2e-18):
        Q = P.copy()
        Q[3] = Q[2] + np.array([np.sqrt(ratio), 0.0, 0.0]) * tmax
        out.append(Q)
    return out


def _lambda_max_legs(L):
    """Collinear legs along x whose second and fourth segments point away from targets R away, so that the spheres' curvature
    -l (d . S) makes the pivot fail until lambda > ~0.35 R / l, while the gradient is exactly zero: the first trial whose pivots
    hold is a step of zero, which is `small`.  R = 4e11: fails through lambda = 1e11, holds at lambda = 1e12 exactly, the last
    value tried, CONVERGED on pass 17.  R = 4e13: fails at every lambda, STALLED in finite arithmetic."""
    out = []
    for R in (4e11, 4e13):
        p0 = np.array([-0.5, -2.0, -1.0])
        out.append(_chain_from(p0, [[R, 0, 0], [-R / 4, 0, 0], [R / 4, 0, 0], [-R / 4, 0, 0]]))
    return out


EDGE_LEGS = {}   # name -> (frame, leg) in the "edges" family, filled by _edges()


def _edges():
    L = base_lengths()
    rng = np.random.default_rng(SEED + 1)
    poses = _tie_poses()
    legs = {}
    u = lo._unit(rng.normal(size=3))
    p0 = np.array([0.3, -1.9, -1.2])
    legs[0] = _chain_from(p0, [L[0][k] * u for k in range(4)])             # straight and exactly reachable
    legs[1] = _chain_from(p0, [2.0 * L[1][k] * u for k in range(4)])       # twice as long as the lengths allow
    v = lo._unit(rng.normal(size=3))
    legs[2] = _chain_from(p0, [0.9 * v, -0.6 * v, 0.8 * v, -0.5 * v])       # consecutive segments antiparallel
    P = _flies(0.02)[0][5, lo.leg_joints(3)].copy()
    P[4] = P[0]                                                             # the tip sits on the anchor
    legs[3] = P
    legs[4], legs[5] = _threshold_legs()
    f = len(poses)
    for leg, name in enumerate(["straight", "too_long", "antiparallel", "tip_on_anchor", "below_tiny", "above_tiny"]):
        EDGE_LEGS[name] = (f, leg)
    poses.append(_pose(rng, legs))
    tried, stall = _lambda_max_legs(L)
    EDGE_LEGS["lambda_max_tried"], EDGE_LEGS["finite_stall"] = (f + 1, 1), (f + 1, 4)
    poses.append(_pose(rng, {1: tried, 4: stall}))
    return np.stack(poses)


# ------------------------------------------------------------------------------------------------------------------ the families
MIXED_KINDS = ("compressed", "easy", "compressed", "noisy")   # frame t of the mixed batch is frame t of family MIXED_KINDS[t % 4]


def _mixed(T=FRAMES):
    """Frames of the compressed, the mildly noisy (0.02) and the noisy (0.5) flies in turn, fitted with the stalled lengths table;
    in three frames of four one leg is missing (a joint of zeros, NaN or infinity in turn)."""
    X5, A, _ = _flies(0.5)
    src = {"compressed": _compressed(X5, A), "easy": _flies(0.02)[0], "noisy": X5}
    X = np.stack([src[MIXED_KINDS[t % 4]][t] for t in range(T)])
    bad = ([0.0, 0.0, 0.0], [1.0, np.nan, 2.0], [-np.inf, 3.0, 1.0])
    for t in range(T):
        if t % 4 != 0:
            X[t, lo.leg_joints((t * 5 + 1) % 6)[1 + t % 4]] = bad[t % 3]
    return X


@functools.lru_cache(maxsize=None)
def families():
    """{name: Family}, in the order the tests run them."""
    L = base_lengths()
    X5, A, _ = _flies(0.5)
    X3 = _flies(0.3)[0]
    rng = np.random.default_rng(SEED + 2)
    offset = A + 3.0 * rng.normal(0.0, 1.0, (6, 3))    # a few lengths
    C = _compressed(X5, A)
    Ls = stalled_lengths()
    out = {
        "noisy": Family(X5, L, A, lo.MAX_ITER), "noisy_free": Family(X5, L, None, lo.MAX_ITER),
        "long": Family(X3, 3.0 * L, A, lo.MAX_ITER), "long_free": Family(X3, 3.0 * L, None, lo.MAX_ITER),
        "long_offset": Family(X3, 3.0 * L, offset, lo.MAX_ITER),
        "short": Family(X3, 0.2 * L, A, lo.MAX_ITER), "short_free": Family(X3, 0.2 * L, None, lo.MAX_ITER),
        "compressed": Family(C, L, A, lo.MAX_ITER), "compressed_free": Family(C, L, None, lo.MAX_ITER),
        "stalled": Family(X5, Ls, A, lo.MAX_ITER), "stalled_free": Family(X5, Ls, None, lo.MAX_ITER),
        "edges": Family(_edges(), L, None, lo.MAX_ITER),
        "tie_step": Family(_pose(np.random.default_rng(SEED + 3), {TIE_SENSITIVE[1]: _tie_sensitive_leg()})[None], L, None, lo.MAX_ITER),
        "milli": Family(1e-3 * X5, 1e-3 * L, 1e-3 * A, lo.MAX_ITER), "kilo": Family(1e3 * X5, 1e3 * L, 1e3 * A, lo.MAX_ITER),
        "shifted": Family(X5 + 1e6, L, None, lo.MAX_ITER),
        "mixed": Family(_mixed(), Ls, A, lo.MAX_ITER), "mixed_free": Family(_mixed(), Ls, None, lo.MAX_ITER),
    }
    for m in sorted(set(LIMITED_FIXED) | set(LIMITED_COUNTS)):
        out[f"limited_{m}"] = Family(X3[:LIMITED_FRAMES], 0.2 * L, A, m)
    for fam in out.values():
        _frozen(fam.X, fam.L, fam.A)
    return out


HARD = ("noisy", "noisy_free", "long", "long_free", "long_offset", "short", "short_free", "compressed", "compressed_free")
LIMITED_FIXED = (1, 2, 3, 7)
LIMITED_FRAMES = 8     # of "short": 48 legs
LIMITED_COUNTS = (3, 4, 5, 6, 7, 8, 9, 10)    # limited_counts(), pinned so that the families have names; the host test recomputes it


def limited_counts():
    """The max_iter values at the boundary: every count n at which a leg of the limited family converges, and n - 1."""
    iters = fit("short").iters[:LIMITED_FRAMES]
    return sorted({int(n) - k for n in np.unique(iters) for k in (0, 1) if int(n) - k >= 1})


def tiled(fam, T):
    """The family's frames repeated to T frames: its period (24, or 8) is no divisor of 64 where T reaches a second wave's frames."""
    return Family(np.ascontiguousarray(fam.X[np.arange(T) % len(fam.X)]), fam.L, fam.A, fam.max_iter)


# ------------------------------------------------------------------------------------------------------------------ the oracle, memoised
Fit = collections.namedtuple("Fit", "points cost status iters traces")
_memo = {}


def fit_family(fam, basis_variant=False):
    """The oracle's fit of a Family, every leg remembered by its inputs' bits with its trace; traces[t][leg] is a list of
    (lam, pivot failed, accepted, small, max |delta|), empty for a leg that is not fitted."""
    X, L = np.asarray(fam.X, dtype=np.float64), np.asarray(fam.L, dtype=np.float64)
    T = len(X)
    out = X.copy()
    E, status, iters = np.full((T, 6), np.nan), np.zeros((T, 6), dtype=np.int32), np.zeros((T, 6), dtype=np.int32)
    traces = [[None] * 6 for _ in range(T)]
    for t in range(T):
        for leg in range(6):
            j = lo.leg_joints(leg)
            a = None if fam.A is None else np.asarray(fam.A, dtype=np.float64)[leg]
            key = (X[t, j].tobytes(), L[leg].tobytes(), None if a is None else a.tobytes(), fam.max_iter, basis_variant)
            if key not in _memo:
                trace = []
                with np.errstate(all="ignore"):   # the overflow leg
                    _memo[key] = lo.fit_leg(X[t, j], L[leg], a, fam.max_iter, basis_variant, trace=trace) + (trace,)
            out[t, j], E[t, leg], status[t, leg], iters[t, leg], traces[t][leg] = _memo[key]
    return Fit(out, E, status, iters, traces)


def fit(name, basis_variant=False):
    return fit_family(families()[name], basis_variant)


def passes(f):
    """[T, 6]: the number of passes (trials) of every leg."""
    return np.array([[len(tr) for tr in row] for row in f.traces])


def leg_scale(fam_scale, P_in, P_want):
    """The factor on a leg's point bar: the family's scale, or the leg's own binade where its coordinates lie beyond FAR."""
    with np.errstate(all="ignore"):
        a = np.abs(np.concatenate([np.ravel(P_in), np.ravel(P_want)]))
    return max(fam_scale, float(2.0 ** (np.floor(np.log2(a[np.isfinite(a)].max())) - 1.0)))


def compare_fits(fam, a, b, converged_flips=True):
    """Two fits of one family, (status [T, 6], iters, points [T, 38, 3], cost) each, b the reference: (differ [T, 6] bool: fitted legs
    whose (status, iters) differ; the largest point difference among the fitted legs that agree, in mm divided by the leg's scale;
    their largest relative cost difference, over costs above RIGID_COST x scale^2).  With `converged_flips` the legs that differ but
    are CONVERGED on both sides count in the two figures as well.  Non-finite values must be of the same class at the same place (inf with inf, NaN with
    NaN) on every leg compared, or an AssertionError names the leg."""
    (sa, ia, pa, ca), (sb, ib, pb, cb) = a, b
    fitted = sb != lo.NOT_FITTED
    differ = ((sa != sb) | (ia != ib)) & fitted
    fs = scale(fam.X)
    dp = dc = 0.0
    both = (sa == lo.CONVERGED) & (sb == lo.CONVERGED) & converged_flips
    for t, leg in zip(*np.nonzero(fitted & (~differ | both))):
        j = lo.leg_joints(leg)
        x, y = pa[t, j], pb[t, j]
        fin = np.isfinite(y)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~fin], y[~fin]), (t, leg, x, y)
        ls = leg_scale(fs, fam.X[t, j], y)
        dp = max(dp, float(np.abs(x[fin] - y[fin]).max()) / ls)
        u, v = float(ca[t, leg]), float(cb[t, leg])
        if np.isfinite(v):
            if v > RIGID_COST * ls * ls:
                dc = max(dc, abs(u - v) / v)
            else:
                assert u <= RIGID_COST * ls * ls, (t, leg, u, v)
        else:
            assert np.isnan(u) == np.isnan(v) and (np.isnan(v) or u == v), (t, leg, u, v)
    return differ, dp, dc


def compare_paths(name):
    """compare_fits of the oracle's two arithmetic paths, basis_variant True against False."""
    a, b = fit(name, basis_variant=True), fit(name)
    return compare_fits(families()[name], (a.status, a.iters, a.points, a.cost), (b.status, b.iters, b.points, b.cost), converged_flips=False)


def bars(name):
    """(point bar in mm per unit of a leg's scale, relative cost bar) of the GPU sweep for a family: see the module's docstring.  After
    one and two iterations (limited_1, limited_2) the floor is STEP_BAR, the bar of tests/test_gpu_leg_fit.py for those counts."""
    _, dp, dc = MEASURED[name]
    return max(10.0 * dp, lo.STEP_BAR if name in ("limited_1", "limited_2") else lo.CONVERGED_BAR), max(10.0 * dc, lo.COST_RTOL)


def overflow_legs(fam):
    """[6] bool: the legs whose squared lengths overflow."""
    return (np.asarray(fam.L) > 1e100).any(axis=1)


# name: (legs that differ between the oracle's two paths; the largest point difference among the others, mm per unit of scale; the
# largest relative cost difference among them).  tests/test_leg_fit_cases_host.py recomputes them
MEASURED = {
    "noisy": (0, 1.110e-15, 7.700e-16),
    "noisy_free": (0, 8.882e-16, 1.088e-15),
    "long": (0, 2.887e-15, 6.727e-16),
    "long_free": (0, 9.437e-15, 5.793e-16),
    "long_offset": (0, 1.776e-15, 3.898e-16),
    "short": (0, 4.441e-16, 2.423e-16),
    "short_free": (0, 2.220e-16, 2.807e-16),
    "compressed": (0, 6.106e-15, 4.927e-16),
    "compressed_free": (0, 3.331e-15, 5.756e-16),
    "stalled": (0, 1.110e-15, 7.700e-16),
    "stalled_free": (0, 8.882e-16, 6.792e-16),
    "edges": (0, 2.220e-16, 1.989e-15),
    "tie_step": (1, 4.441e-16, 3.706e-15),   # the one leg is TIE_SENSITIVE: the other basis is another model of `small` there
    "milli": (0, 1.332e-15, 6.510e-16),
    "kilo": (0, 8.882e-16, 1.413e-15),
    "shifted": (0, 0.000e+00, 7.877e-16),    # both paths round to the same unit in the last place of 1e6 mm
    "mixed": (0, 6.106e-15, 1.479e-15),
    "mixed_free": (0, 2.442e-15, 6.760e-15),
    "limited_1": (0, 2.220e-16, 2.742e-16),
    "limited_2": (0, 6.661e-16, 4.366e-16),
    "limited_3": (0, 2.220e-16, 2.513e-16),
    "limited_4": (0, 2.220e-16, 2.221e-16),
    "limited_5": (0, 2.220e-16, 2.389e-16),
    "limited_6": (0, 2.220e-16, 2.745e-16),
    "limited_7": (0, 2.220e-16, 2.221e-16),
    "limited_8": (0, 2.220e-16, 2.221e-16),
    "limited_9": (0, 2.220e-16, 2.221e-16),
    "limited_10": (0, 2.220e-16, 2.221e-16),
}
