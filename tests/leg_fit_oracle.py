"""Float64 restatement of the constant-length leg fit, one leg at a time in plain numpy: a damped Newton
method on the product of four unit spheres that fits a chain of fixed segment lengths to the measured joints of a leg.  The model is
this project's own specification; this module defines it.  `basis_variant=True` builds every tangent basis from the coordinate axis
AFTER the largest component of the direction instead of the axis of the smallest one: the same model on another arithmetic path,
which measures how far the converged answer depends on rounding.  `fit_leg(trace=[])` records every pass.  `replay` is the closed form of max_iter = 0, `witness_fit` an
independent scipy fit of the same cost in spherical angles."""
import numpy as np

TINY = 1e-18         # relative bound on a squared start segment below which its direction is undefined
TOL = 1e-9           # a step whose largest tangent coordinate is at most this ends the iteration
SLACK = 1e-12        # a trial is accepted when E' <= E (1 + SLACK): see fit_leg
LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e12
MAX_ITER = 30
NOT_FITTED, CONVERGED, OUT_OF_ITERATIONS, STALLED = -1, 0, 1, 2

# Bars of the tests, in mm on millimetre-sized coordinates: ten times what was measured on an MI355X.
# STEP_BAR: kernel against oracle after zero, one and two iterations, where both take the same steps and only rounding differs:
# 8.9e-16 measured, two units in the last place of a coordinate.  CONVERGED_BAR: the larger of the kernel-to-oracle difference at the
# default max_iter (1.33e-15 over every case of tests/test_gpu_leg_fit.py, the iteration counts equal everywhere) and the oracle's
# own sensitivity to the tangent basis (8.9e-16 on the golden and on the synthetic set).  COST_RTOL: the same factor on the largest
# relative difference of a cost (8.5e-13).
STEP_BAR = 8.9e-15
CONVERGED_BAR = 1.33e-14
COST_RTOL = 8.5e-12


def leg_joints(leg):
    side, l = divmod(leg, 3)
    return [19 * side + 5 * l + k for k in range(5)]


def missing(p):
    """All three coordinates exactly 0, or any of them not finite (section 14's rule)."""
    p = np.asarray(p, dtype=np.float64)
    return bool(np.all(p == 0.0) or not np.all(np.isfinite(p)))


def start(P, anchor=None):
    """(p0 [3], t [4, 3] targets, d [4, 3] start directions), or None when the leg is not fitted."""
    P = np.asarray(P, dtype=np.float64)
    if any(missing(P[k]) for k in range(1, 5)):
        return None
    if anchor is None:
        if missing(P[0]):
            return None
        p0 = P[0].copy()
    else:
        p0 = np.asarray(anchor, dtype=np.float64).copy()
        if not np.all(np.isfinite(p0)):
            return None
    with np.errstate(over="ignore", invalid="ignore"):
        t = P[1:] - p0
        s = np.concatenate([t[:1], t[1:] - t[:-1]])
        tmax = max(float(x @ x) for x in t)
        ss = np.array([x @ x for x in s])
        if not np.all(ss > TINY * tmax):   # also refuses a NaN
            return None
        return p0, t, s / np.sqrt(ss)[:, None]


def chain(d, lengths):
    """c [4, 3]: c_k = sum_{i <= k} l_i d_i."""
    c = np.zeros((4, 3))
    acc = np.zeros(3)
    for k in range(4):
        acc = acc + lengths[k] * d[k]
        c[k] = acc
    return c


def cost(d, lengths, t):
    r = chain(d, lengths) - t
    return float(sum(x @ x for x in r))


def tangent_basis(d, basis_variant=False):
    """B [3, 2] = [b1 b2]: b1 = (d x e)/|d x e|, b2 = d x b1, e a coordinate axis."""
    a = np.abs(d)
    axis = (int(np.argmax(a)) + 1) % 3 if basis_variant else int(np.argmin(a))   # argmin / argmax: ties go to the lowest index
    e = np.zeros(3)
    e[axis] = 1.0
    b1 = np.cross(d, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return np.stack([b1, np.cross(d, b1)], axis=1)


def cholesky_solve(A, b):
    """x with A x = b by an unpivoted Cholesky factorisation, or None at the first pivot that is not > 0."""
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        p = A[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0.0:
            return None
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def fit_leg(P, lengths, anchor=None, max_iter=MAX_ITER, basis_variant=False, trace=None):
    """(points [5, 3], cost, status, iterations) of one leg: joints P [5, 3], fixed lengths [4], anchor [3] or None.  A list given as
    `trace` receives one record per pass (one trial): (lam, pivot failed, accepted, small, max |delta|); where the pivot failed `small` is
    False and max |delta| NaN.  The trace only listens: the results are the same bits with and without it."""
    P = np.asarray(P, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64)
    st = start(P, anchor)
    if st is None:
        return P.copy(), np.nan, NOT_FITTED, -1
    p0, t, d = st
    lam, iters = 0.0, 0
    status = OUT_OF_ITERATIONS if max_iter == 0 else None
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while status is None:
            r = chain(d, lengths) - t
            S = np.stack([r[i:].sum(axis=0) for i in range(4)])
            E = float(sum(x @ x for x in r))
            B = [tangent_basis(d[i], basis_variant) for i in range(4)]
            g = np.concatenate([lengths[i] * (B[i].T @ S[i]) for i in range(4)])
            H = np.zeros((8, 8))
            D = np.zeros(8)
            for i in range(4):
                for j in range(4):
                    H[2 * i:2 * i + 2, 2 * j:2 * j + 2] = lengths[i] * lengths[j] * (4 - max(i, j)) * (B[i].T @ B[j])
                H[2 * i:2 * i + 2, 2 * i:2 * i + 2] -= lengths[i] * (d[i] @ S[i]) * np.eye(2)
                D[2 * i:2 * i + 2] = lengths[i] * lengths[i] * (4 - i)
            while True:
                delta = cholesky_solve(H + lam * np.diag(D), -g)
                accepted = small = False
                step = np.nan
                if delta is not None:
                    trial = np.stack([d[i] + B[i] @ delta[2 * i:2 * i + 2] for i in range(4)])
                    trial = trial / np.sqrt((trial * trial).sum(axis=1))[:, None]
                    small = bool(np.all(np.abs(delta) <= TOL))
                    step = float(np.abs(delta).max()) if trace is not None else np.nan
                    # the slack: E is a sum of twelve squares, good to ~1e-15 relative.  A plain E' < E fails by rounding on a
                    # last step of ~3e-9, the damping then grows until the step shrinks under TOL, and the leg "converges" 1e-9 mm
                    # short; which legs do depends on the arithmetic path (basis_variant moved the answer by 1.1e-9 mm, with the
                    # slack by 9e-16), and the iteration counts are the same
                    accepted = small or cost(trial, lengths, t) <= E * (1.0 + SLACK)
                if trace is not None:
                    trace.append((lam, delta is None, accepted, small, step))
                if accepted:
                    break
                lam = max(10.0 * lam, LAMBDA_MIN)
                if lam > LAMBDA_MAX:
                    status = STALLED
                    break
            if status is not None:
                break
            d = trial
            iters += 1
            lam = lam / 10.0 if lam > LAMBDA_MIN else 0.0
            if small:
                status = CONVERGED
            elif iters == max_iter:
                status = OUT_OF_ITERATIONS
    c = chain(d, lengths)
    r = c - t
    return np.concatenate([p0[None], p0 + c]), float(sum(x @ x for x in r)), status, iters


def fit_legs(X, lengths, anchor=None, max_iter=MAX_ITER, basis_variant=False):
    """X [T, 38, 3], lengths [6, 4], anchor [6, 3] or None -> (points [T, 38, 3], cost [T, 6], status [T, 6], iterations [T, 6]);
    the eight joints that belong to no leg are copied."""
    X = np.asarray(X, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64)
    T = len(X)
    out = X.copy()
    E, status, iters = np.full((T, 6), np.nan), np.zeros((T, 6), dtype=np.int32), np.zeros((T, 6), dtype=np.int32)
    for t in range(T):
        for leg in range(6):
            j = leg_joints(leg)
            out[t, j], E[t, leg], status[t, leg], iters[t, leg] = fit_leg(X[t, j], lengths[leg], None if anchor is None else anchor[leg], max_iter,
                                                                          basis_variant)
    return out, E, status, iters


def replay(P, lengths, anchor=None):
    """[5, 3]: the measured directions replayed with the fixed lengths, what max_iter = 0 returns (P itself when not fitted)."""
    st = start(P, anchor)
    if st is None:
        return np.asarray(P, dtype=np.float64).copy()
    p0, _, d = st
    return np.concatenate([p0[None], p0 + np.cumsum(np.asarray(lengths)[:, None] * d, axis=0)])


# ------------------------------------------------------------------------------------------------------------------ inputs
def segment_lengths(X):
    """[T, 6, 4] with NaN where an end joint is missing (section 14's lengths)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.full((len(X), 6, 4), np.nan)
    for t in range(len(X)):
        for leg in range(6):
            P = X[t, leg_joints(leg)]
            for k in range(4):
                if not missing(P[k]) and not missing(P[k + 1]):
                    v = P[k + 1] - P[k]
                    out[t, leg, k] = np.sqrt(v @ v)
    return out


def median_lengths(X):
    """[6, 4]: the median over the frames of every segment's finite lengths."""
    L = segment_lengths(X)
    L[~np.isfinite(L)] = np.nan
    return np.nanmedian(L, axis=0)


COXAE = [0, 5, 10, 19, 24, 29]


def recording_anchor(X):
    """[6, 3]: the temporal medians of the six body-coxa joints over all frames as they stand."""
    return np.median(np.asarray(X, dtype=np.float64)[:, COXAE], axis=0)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, [1, 0, 2]]


def _unit(v):
    return v / np.sqrt(v @ v)


def synthetic_flies(rng, T, lengths, noise=0.02):
    """(X [T, 38, 3], anchor [6, 3], rigid [T, 38, 3]): legs of exactly the lengths [6, 4] hanging from six fixed body-coxa positions in
    random directions (consecutive segments bent by at least ~0.2 rad), `rigid`; X adds Gaussian noise of `noise` x the mean length to
    every joint; the anchor is the true body-coxa position plus an offset of the same size.  The other eight joints hold noise."""
    lengths = np.asarray(lengths, dtype=np.float64)
    sigma = noise * float(lengths.mean())
    base = rng.uniform(-1.0, 1.0, (6, 3))
    rigid = rng.normal(0.0, 1.0, (T, 38, 3))
    for t in range(T):
        for leg in range(6):
            P = [base[leg]]
            d = _unit(rng.normal(size=3))
            for k in range(4):
                if k:
                    while True:
                        nxt = _unit(rng.normal(size=3))
                        if abs(nxt @ d) < 0.98:
                            break
                    d = nxt
                P.append(P[-1] + lengths[leg, k] * d)
            rigid[t, leg_joints(leg)] = np.stack(P)
    X = rigid.copy()
    legs = [j for leg in range(6) for j in leg_joints(leg)]
    X[:, legs] += rng.normal(0.0, sigma, (T, 30, 3))
    anchor = base + rng.normal(0.0, sigma, (6, 3))
    return X, anchor, rigid


# ------------------------------------------------------------------------------------------------------------------ the scipy witness
def witness_fit(P, lengths, anchor=None):
    """(points [5, 3], cost): scipy's Levenberg-Marquardt on the same residuals with every direction written as
    (cos el cos az, cos el sin az, sin el) in a frame turned so that the start direction sits at el = az = 0 (no pole nearby),
    started from the same directions."""
    from scipy.optimize import least_squares

    p0, t, d0 = start(P, anchor)
    lengths = np.asarray(lengths, dtype=np.float64)
    frames = []
    for d in d0:
        B = tangent_basis(d)
        frames.append(np.stack([d, B[:, 0], B[:, 1]], axis=1))   # columns: the start direction and two perpendiculars

    def directions(x):
        out = []
        for i in range(4):
            el, az = x[2 * i], x[2 * i + 1]
            out.append(frames[i] @ np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)]))
        return np.stack(out)

    def residuals(x):
        return (chain(directions(x), lengths) - t).ravel()

    def jacobian(x):   # d r_k / d (el_i, az_i) = l_i d d_i / d (el_i, az_i) for k >= i
        J = np.zeros((4, 3, 8))
        for i in range(4):
            el, az = x[2 * i], x[2 * i + 1]
            d_el = frames[i] @ np.array([-np.sin(el) * np.cos(az), -np.sin(el) * np.sin(az), np.cos(el)])
            d_az = frames[i] @ np.array([-np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), 0.0])
            J[i:, :, 2 * i] = lengths[i] * d_el
            J[i:, :, 2 * i + 1] = lengths[i] * d_az
        return J.reshape(12, 8)

    sol = least_squares(residuals, np.zeros(8), jac=jacobian, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    c = chain(directions(sol.x), lengths)
    r = c - t
    return np.concatenate([p0[None], p0 + c]), float(sum(x @ x for x in r))
