"""Seeded inputs for the trajectory triangulation (csrc/trajectory.hip): points on planted smooth trajectories in
front of the rig of tests/pose_chain_cases.py, projected exactly and snapped to the 7.5 px cells of a heat-map; the named families of
the sweep (sweep(), at the end) with the three-path certificate of their chains (decisions()).  Host numpy only.
TEST INFRASTRUCTURE ONLY."""
import collections
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


def reference(P, px, X0):
    """The oracle in float64 and in numpy.longdouble from the device's own start at config's defaults, how far rounding alone moves it,
    and the bar on X."""
    import trajectory_oracle as to
    from deepfly3d_amd import config

    lam = config.TRAJECTORY_LAMBDA[: px.shape[2]]
    r64 = to.fit(P, px, X0, lam, config.TRAJECTORY_HUBER, config.REPAIR_MAX_GAP)
    r80 = to.fit(P, px, X0, lam, config.TRAJECTORY_HUBER, config.REPAIR_MAX_GAP, dtype=np.longdouble)
    moved = float(np.abs(r64["X"] - r80["X"].astype(np.float64)).max())
    return r64, r80, moved, max(16.0 * moved, config.TRAJECTORY_STEP_TOL)


def error_and_cost_bars(P, px, r64, lam, delta, bar):
    """What a point within `bar` (mm, per coordinate) of the oracle's may change, derived and not measured:
    a view's error e = |proj(X) - px| moves by at most |J_c|_2 |dX|_2 <= L sqrt(3) bar, L^2 = the largest trace of a frame's sum of
    J^T J at the oracle's point (it bounds every view's |J_c|_2^2 there; doubled for J's own change over `bar`), plus 16 eps e for the
    rounding of the projection; a view's Huber term has slope at most 2 delta, a triple's |s|^2 moves by at most 2 |s|_2 |ds|_2 +
    |ds|_2^2 with |ds|_2 <= 4 sqrt(3) bar; the chain sum of at most T ncam + T terms rounds within 1e-12 of the cost.
    Returns (error bar [ncam, T, J], cost bar [J])."""
    import trajectory_oracle as to

    eps = np.finfo(np.float64).eps
    H = to.linearize(P, px, r64["X"], np.inf)[0]
    L = float(np.sqrt(np.nanmax(H[..., 0] + H[..., 3] + H[..., 5])))
    moved = 2.0 * np.sqrt(3.0) * L * bar
    with np.errstate(invalid="ignore"):
        error_bar = moved + 16.0 * eps * np.where(np.isfinite(r64["error"]), r64["error"], 0.0)
    views = (to.views(px) & r64["active"][None]).sum(axis=(0, 1))
    s = np.linalg.norm(to.smoothness(r64["X"], r64["centre"])[0], axis=-1)
    ds = 4.0 * np.sqrt(3.0) * bar
    cost_bar = 2.0 * delta * views * moved + lam * (2.0 * s * ds + ds * ds).sum(axis=0) + 1e-12 * r64["cost"][:, 1]
    return error_bar, cost_bar


# ---- the sweep of the damped branch, long chains and shapes ("swept") ------------------------------------------
# A family is one launch.  `firm` names the chains whose every decision the oracle takes alike along three paths (decisions()); those
# a GPU test asserts exactly.  `structural` names the chains whose end does not depend on rounding at all (a NaN pivot, a NaN cost):
# their certificate is the float64 oracle and the argument in the builder's docstring.  Every other chain is compared in invariants only.
Sweep = collections.namedtuple("Sweep", "P px X0 lam huber max_gap firm structural")
NOISE_MM = 50.0
HUGE = 1.7e308
PATHS = ("float64", "longdouble", "dense")
SWEEP_FAMILIES = ("rejected", "rejected_clean", "out_of_iterations", "pivot_stall", "nan_cost_stall", "per_joint_lambda", "cost_stalled",
                  "mixed", "long", "segments0", "segments1", "segments2", "segments5", "cameras2", "cameras8")


def _sweep(P, px, X0, lam, huber, max_gap, firm=(), structural=()):
    J = px.shape[2]
    out = Sweep(np.ascontiguousarray(P), np.ascontiguousarray(px), np.ascontiguousarray(X0),
                np.ascontiguousarray(np.broadcast_to(np.asarray(lam, np.float64), (J,))), float(huber), int(max_gap), tuple(firm), tuple(structural))
    for a in out[:4]:
        a.setflags(write=False)
    return out


def _noisy_start(P, px, seed):
    return dlt(P, px) + np.random.default_rng([9, seed]).normal(0.0, NOISE_MM, size=px.shape[1:3] + (3,))


def _long(J):
    """T = 1025 (342 blocks of 3: the lanes 0 .. 85 take two; a lane's setup chunk is five frames), three views.  Camera 0 alone in
    eight frames from 52, 333, 598 and 1001 (each crosses the chunks of two or three lanes), no view at all in 700 .. 705 (status 3),
    one view in the first seven frames and none in the last nine: neither end has an anchor to close it."""
    P, px, _ = _detections(1025, 2, range(3), 3)
    for s in (52, 333, 598, 1001):
        px[1:3, s : s + GAP_LEN] = 0.0
    px[:, 700:706] = 0.0
    px[1:, :7] = 0.0
    px[:, 1016:] = 0.0
    px = np.ascontiguousarray(px[:, :, :J])
    return _sweep(P, px, dlt(P, px), LAMBDA, HUBER, 10, firm=range(J))


def _segments(max_gap):
    """T = 64, J = 64, clean three-view data at the defaults.  Chain j alternates runs of anchors of 2, 3, 4, 5 or 7 frames with gaps of
    1, 2, 3, 5 or 6 frames, in an order of its own: a gap either side of each max_gap in (0, 1, 2, 5).  A gap's frames keep camera 0
    (status 2) or no camera (status 3), by turns.  Chains with j % 2 == 0 start at an anchor and those with j % 3 == 0 end at one; the
    others start or end inside a gap that nothing closes."""
    T, J = 64, 64
    P, px, _ = _detections(T, J, range(3), 5)
    for j in range(J):
        rng = np.random.default_rng([53, j])
        t, k = (0 if j % 2 == 0 else -int(rng.integers(1, 4))), 0
        anchor = np.zeros(T, bool)
        while t < T:
            run = int(rng.choice((2, 3, 4, 5, 7)))
            anchor[max(t, 0) : t + run] = True
            t += run + int(rng.choice((1, 2, 3, 5, 6)))
        if j % 3 == 0:
            anchor[T - 1] = True
        else:
            anchor[T - 2 :] = False
        for t in np.nonzero(~anchor)[0]:
            px[(1 if (k + t) % 2 else 0):, t, j] = 0.0
            k += 1
    return _sweep(P, px, dlt(P, px), LAMBDA, HUBER, max_gap, firm=range(J))


def _cameras(ncam):
    P = rig(ncam)
    px = quantise(project(P, sinusoid(24, 2, seed=2)))
    px[3:] = 0.0
    return _sweep(P, px, dlt(P, px), LAMBDA, HUBER, 10, firm=range(2))


@functools.lru_cache(maxsize=None)
def sweep(name):
    """The family `name` of SWEEP_FAMILIES, a Sweep.  Read only.
    rejected, rejected_clean   a start N(0, 50 mm) beside the plain triangulation: chain 1 converges after 66 of 119 (6 of 16) trials
                               were rejected on cost
    out_of_iterations          huber = 1e-6 px: chain 0 is accepted 300 times and would need more than 600 trials; chain 1 converges
    pivot_stall                lambda = 1e308, finite: lambda k1 = -2 lambda (c(t) + c(t + 1)) is -inf wherever two centres meet, and so is
                               a multiplier of the first pivot eliminated beside it in any order; the next pivot is inf - inf.  16
                               trials, all rejected at a pivot
    nan_cost_stall             chain 0: two anchors at +-1.7e308 around a bridged frame; B - A overflows, the start holds -inf, the cost
                               of the start and of every trial is NaN and no NaN is <= anything: 16 trials, all rejected on cost
    per_joint_lambda           lambda = (0, 1e5)
    cost_stalled               the start of another seed: chain 1 stalls on cost after about a hundred trials and the three paths take
                               different sequences.  Not firm, on purpose
    mixed                      huber = 1e-6, one lambda per chain: converged after rejections, out of iterations, converged without a
                               rejection, stalled at a pivot, no active frame
    long, segments<max_gap>, cameras<ncam>: _long, _segments, _cameras"""
    if name in ("rejected", "cost_stalled"):
        P, px = fit_case("gaps", 40)
        return _sweep(P, px, _noisy_start(P, px, 2 if name == "rejected" else 4), LAMBDA, 2.0, 10, firm=(0, 1) if name == "rejected" else (0,))
    if name == "rejected_clean":
        P, px = fit_case("clean2", 24)
        return _sweep(P, px, _noisy_start(P, px, 2), 0.0, HUBER, 10, firm=(0, 1))
    if name in ("out_of_iterations", "pivot_stall"):
        P, px = fit_case("outliers3", 24)
        if name == "pivot_stall":
            return _sweep(P, px, dlt(P, px), 1e308, 1e-6, 10, structural=(0, 1))
        return _sweep(P, px, dlt(P, px), LAMBDA, 1e-6, 10, firm=(0, 1))
    if name == "nan_cost_stall":
        P, px = fit_case("clean3", 24)
        px, X0 = np.array(px), np.array(dlt(P, px))
        px[1:, 10, 0] = 0.0           # one view: no anchor, bridged
        X0[9, 0], X0[11, 0] = HUGE, -HUGE
        return _sweep(P, px, X0, LAMBDA, HUBER, 10, firm=(1,), structural=(0,))
    if name == "per_joint_lambda":
        P, px = fit_case("outliers3", 40)
        return _sweep(P, px, dlt(P, px), (0.0, 1e5), HUBER, 10, firm=(0, 1))
    if name == "mixed":
        P, noisy = fit_case("clean2", 24)
        plain = fit_case("outliers3", 24)[1]
        px = np.concatenate([noisy[:, :, :1], plain, plain[:, :, 1:], np.zeros_like(plain[:, :, :1])], axis=2)
        X0 = np.concatenate([_noisy_start(P, noisy, 2)[:, :1], dlt(P, px[:, :, 1:])], axis=1)
        return _sweep(P, px, X0, (0.0, LAMBDA, LAMBDA, 1e308, 7.0), 1e-6, 10, firm=(0, 1, 2, 4), structural=(3,))
    if name == "long":
        return _long(2)
    if name.startswith("segments"):
        return _segments(int(name[8:]))
    if name.startswith("cameras"):
        return _cameras(int(name[7:]))
    raise KeyError(name)


def _dense_solve(AB, b):
    """The third path: numpy.linalg.solve (LU with partial pivoting) on the dense matrix for the step; ok still from the banded pivots."""
    import trajectory_oracle as to

    with np.errstate(all="ignore"):
        return np.linalg.solve(to.dense(AB), b[..., None])[..., 0], to.banded_solve(AB, b)[1]


Decisions = collections.namedtuple("Decisions", "strings fit_status results firm spread cost_margin step_margin")


def decisions(P, px, X0, lam, huber, max_gap, max_iter=None, paths=PATHS):
    """The oracle along `paths` (float64, numpy.longdouble, float64 with the dense solve).  Returns
    strings      {path: [J] str}, a letter per trial: a accepted, c rejected on cost, p rejected at a pivot
    fit_status   {path: [J]}, results {path: the oracle's dict}
    firm         [J] bool: every path takes the same decisions and ends alike
    spread       [J]: the largest |X - X'| between two paths (NaN where a path holds a non-finite point)
    cost_margin  [J]: the smallest |En - E (1 + SLACK)| / E of float64's cost decisions (trials whose pivots held and whose step was
                 not small), inf where there was none or the cost is NaN
    step_margin  [J]: the smallest |max |d| - STEP_TOL| / STEP_TOL of float64's trials whose pivots held"""
    import trajectory_oracle as to
    from deepfly3d_amd import config

    J = px.shape[2]
    strings, status, results, traces = {}, {}, {}, {}
    for path in paths:
        traces[path] = []
        results[path] = to.fit(P, px, X0, lam, huber, max_gap, dtype=np.longdouble if path == "longdouble" else np.float64, max_iter=max_iter,
                               solve=_dense_solve if path == "dense" else None, trace=traces[path])
        s = [""] * J
        for trial in traces[path]:
            for i, k in enumerate(trial["chains"]):
                s[k] += "a" if trial["accept"][i] else "c" if trial["ok"][i] else "p"
        strings[path], status[path] = s, results[path]["fit_status"]
    first = paths[0]
    firm = np.array([all(strings[p][j] == strings[first][j] and status[p][j] == status[first][j] for p in paths) for j in range(J)])
    spread = np.zeros(J)
    for a in range(len(paths)):
        for b in range(a + 1, len(paths)):
            spread = np.maximum(spread, np.abs(results[paths[a]]["X"].astype(np.float64) - results[paths[b]]["X"].astype(np.float64)).max(axis=(0, 2)))
    cost_margin, step_margin = np.full(J, np.inf), np.full(J, np.inf)
    tol, slack = config.TRAJECTORY_STEP_TOL, config.TRAJECTORY_SLACK
    with np.errstate(all="ignore"):
        for trial in traces["float64"] if "float64" in traces else ():
            k, E, En, step = trial["chains"], trial["E"].astype(np.float64), trial["En"].astype(np.float64), trial["step"].astype(np.float64)
            cm = np.where(trial["ok"] & ~trial["small"], np.abs(En - E * (1.0 + slack)) / E, np.inf)
            cost_margin[k] = np.fmin(cost_margin[k], np.where(np.isnan(cm), np.inf, cm))
            sm = np.where(trial["ok"], np.abs(step - tol) / tol, np.inf)
            step_margin[k] = np.fmin(step_margin[k], np.where(np.isnan(sm), np.inf, sm))
    return Decisions(strings, status, results, firm, spread, cost_margin, step_margin)


@functools.lru_cache(maxsize=None)
def certificate(name):
    """decisions() of the family `name`: its firm chains along the three paths, as a launch of their own (a chain's fit does not
    depend on its company), and the whole launch in float64 (`.whole`, the oracle's dict)."""
    import trajectory_oracle as to

    fam = sweep(name)
    k = list(fam.firm)
    three = decisions(fam.P, fam.px[:, :, k], fam.X0[:, k], fam.lam[k], fam.huber, fam.max_gap) if k else None
    if k == list(range(fam.px.shape[2])):
        whole = three.results["float64"]
    else:
        whole = to.fit(fam.P, fam.px, fam.X0, fam.lam, fam.huber, fam.max_gap)
    return CERT(tuple(k), three, whole)


CERT = collections.namedtuple("CERT", "firm_chains three whole")


def chains_of(fam, k):
    """The chains k of a family as a launch of their own."""
    k = list(k)
    return _sweep(fam.P, fam.px[:, :, k], fam.X0[:, k], fam.lam[k], fam.huber, fam.max_gap)


def result_of(r, k):
    """The chains k of an oracle's dict."""
    k = list(k)
    first = {"X": 1, "status": 1, "weight": 2, "error": 2, "active": 1, "centre": 1, "anchor": 1}
    return {key: (v[:, k] if first.get(key) == 1 else v[:, :, k] if first.get(key) == 2 else v[k]) for key, v in r.items()}


def point_bar(name):
    """The bar on a firm chain's points: max(16 x the largest difference between two of the three paths, STEP_TOL), per family."""
    from deepfly3d_amd import config

    return max(16.0 * float(certificate(name).three.spread.max()), config.TRAJECTORY_STEP_TOL)
