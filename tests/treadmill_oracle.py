"""Float64 statement of the treadmill model in plain numpy, one IEEE operation at a time: the leg tips and
their velocities in the recording's body frame, one sphere through the stance samples (algebraic, or Gauss-Newton with a known
radius), the ball's rotation in every frame, the fly's fictive motion and its path.  The model is this project's own specification;
it claims no parity with anything.  The model's sums are exact (math.fsum); `sums_kernel_form` restates them in the order of
csrc/treadmill.hip.  Also here: the bars of the floating-point comparisons with their derivations, and the planted ball."""
import math

import numpy as np

import gait_oracle as go
import joint_angles_oracle as jo

HALF = go.HALF                      # config.GAIT_DIFF_HALF
ITERATIONS = 8                      # config.BALL_FIT_ITERATIONS
PIVOT_MIN = 1e-10                   # config.BALL_PIVOT_MIN
MIN_LEGS = 2                        # config.BALL_MIN_LEGS
FRAME_PIVOT_MIN = 1e-10             # config.BALL_FRAME_PIVOT_MIN
SLICE, THREADS, WAVE = 2048, 256, 64   # constants of csrc/treadmill.hip: the samples (t, L) of one sum slice, a block's lanes, a wave
S = SLICE
SCAN_BLOCK = THREADS                # the frames of one block of the scan
B = THREADS * THREADS               # the frames at which the scan's second level first needs a second block of block results
U = go.U
REFUSED, START_BELOW = 1, 2         # the bits of the status word
TIPS, COXAE = go.TIPS, go.COXAE
missing = go.missing
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------ stage 1: the tips
def coxa_medians(X):
    """[6, 3]: the temporal medians of the six body-coxa joints over all frames as they stand."""
    return np.median(np.asarray(X, dtype=np.float64)[:, COXAE], axis=0)


def origin(medians):
    """The six medians summed in leg order, then one division."""
    o = medians[0]
    for k in range(1, 6):
        o = o + medians[k]
    return o / 6.0


def in_frame(v, F):
    """F v of v [..., 3]: every dot product as x x + y y + z z from the left."""
    return np.stack([v[..., 0] * F[r, 0] + v[..., 1] * F[r, 1] + v[..., 2] * F[r, 2] for r in range(3)], axis=-1)


def body_tips(X, fps, F, medians, w=HALF):
    """X [T, 38, 3], the frame F [3, 3] and the medians [6, 3] -> (b [T, 6, 3], v [T, 6, 3])."""
    X = np.asarray(X, dtype=np.float64)
    T = len(X)
    if T == 0:
        return np.zeros((0, 6, 3)), np.zeros((0, 6, 3))
    F = np.asarray(F, dtype=np.float64)
    o = origin(np.asarray(medians, dtype=np.float64))
    frame_ok = bool(np.all(np.isfinite(F)) and np.all(np.isfinite(o)))
    lo, hi = go.window(T, w)
    P4 = X[:, TIPS]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        b = in_frame(P4 - o, F)
        scale = (fps / (hi - lo).astype(np.float64))[:, None, None]   # one division
        v = in_frame(P4[hi] - P4[lo], F) * scale
    b[~(frame_ok & ~missing(P4))] = np.nan
    v[~(frame_ok & (hi > lo)[:, None] & ~missing(P4[lo]) & ~missing(P4[hi]))] = np.nan
    return b, v


# ------------------------------------------------------------------------------------------------------------------ stage 2: the ball
def samples(b, states):
    """[T, 6] bool: a stance state with a finite tip."""
    return (np.asarray(states) == 0) & np.all(np.isfinite(b), axis=-1)


def exact_sum(x, keep):
    return math.fsum(x[keep].tolist())


def slice_sum(x, keep):
    """The sum of x [n] where `keep`, in the order of ball_sums_kernel and its fold: a lane's eight samples of a slice in order, the
    shuffle tree over a wave, the four waves in order, the slices in order.  A sample left out adds +0.0, which changes no bit."""
    n = len(x)
    slices = (n + SLICE - 1) // SLICE
    full = np.zeros(slices * SLICE)
    full[:n] = np.where(keep, x, 0.0)
    full = full.reshape(slices, SLICE)
    lanes = np.zeros((slices, THREADS))
    for k in range(SLICE // THREADS):
        lanes = lanes + full[:, k * THREADS:(k + 1) * THREADS]
    waves = lanes.reshape(slices, THREADS // WAVE, WAVE).copy()
    o = WAVE // 2
    while o:
        waves[..., :o] = waves[..., :o] + waves[..., o:2 * o]
        o //= 2
    total = waves[:, 0, 0]
    for w in range(1, THREADS // WAVE):
        total = total + waves[:, w, 0]
    out = 0.0
    for part in total:
        out = out + part
    return float(out)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def ball_sums(b, states, total=exact_sum):
    """[17]: the count, the sum of b [3], and with m = that sum / count and q = b - m the 13 sums of the centred normal equations, in
    the order of include/df3d_hip.h."""
    keep = samples(b, states).reshape(-1)
    flat = np.where(keep[:, None], np.asarray(b, dtype=np.float64).reshape(-1, 3), 0.0)
    n = float(keep.sum())
    out = [n] + [total(flat[:, k], keep) for k in range(3)]
    if n == 0.0:
        return np.array(out + [0.0] * 13)
    m = np.array(out[1:4]) / n
    q = flat - m
    w = _dot(q, q)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    terms = (x * x, x * y, x * z, x, y * y, y * z, y, z * z, z, x * w, y * w, z * w, w)
    return np.array(out + [total(t, keep) for t in terms])


def sums_kernel_form(b, states):
    """ball_sums in the order of the device: what df3d_ball_fit reports in `sums`, bit for bit."""
    return ball_sums(b, states, slice_sum)


def normal4(s):
    """(A [4, 4], rhs [4]) of the 17 sums: rows (qx, qy, qz, 1), right side |q|^2."""
    n, (xx, xy, xz, x, yy, yz, y, zz, z) = s[0], s[4:13]
    A = np.array([[xx, xy, xz, x], [xy, yy, yz, y], [xz, yz, zz, z], [x, y, z, n]])
    return A, np.array(s[13:17])


def cholesky_solve(A, rhs, floor, seen=None):
    """The solution of A p = rhs by Cholesky, row by row as the kernels do; None where a pivot is at or below `floor` or no number.
    `seen`: a list that takes (pivot, floor) of every pivot decision, up to and with the first refused one."""
    k = len(rhs)
    L = np.zeros((k, k))
    for i in range(k):
        for j in range(i + 1):
            acc = A[i, j]
            for c in range(j):
                acc = acc - L[i, c] * L[j, c]
            if i == j:
                if seen is not None:
                    seen.append((float(acc), float(floor)))
                if not acc > floor:
                    return None
                L[i, i] = math.sqrt(acc)
            else:
                L[i, j] = acc / L[j, j]
    y = np.zeros(k)
    for i in range(k):
        acc = rhs[i]
        for c in range(i):
            acc = acc - L[i, c] * y[c]
        y[i] = acc / L[i, i]
    p = np.zeros(k)
    for i in reversed(range(k)):
        acc = y[i]
        for c in range(i + 1, k):
            acc = acc - L[c, i] * p[c]
        p[i] = acc / L[i, i]
    return p


def _algebraic(s, seen=None):
    """(centre [3], radius) of the 17 sums, or None where the fit is refused."""
    n = s[0]
    if n < 4.0:
        return None
    A, rhs = normal4(s)
    p = cholesky_solve(A, rhs, PIVOT_MIN * float(np.max(np.diag(A))), seen)
    if p is None:
        return None
    a = 0.5 * p[:3]
    R2 = p[3] + (a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    if not (R2 > 0.0 and np.isfinite(R2) and np.all(np.isfinite(a))):
        return None
    return a + s[1:4] / n, math.sqrt(R2)


def step_sums(b, states, c, R, total=exact_sum):
    """[10]: with d = b - c, rho = |d|, u = d / rho and r = rho - R: sum ux ux, ux uy, ux uz, uy uy, uy uz, uz uz, ux r, uy r, uz r (over
    the samples with rho > 0) and r r (over all samples)."""
    keep = samples(b, states).reshape(-1)
    d = np.where(keep[:, None], np.asarray(b, dtype=np.float64).reshape(-1, 3), 0.0) - c
    rho = np.sqrt(_dot(d, d))
    r = rho - R
    dir_ok = keep & (rho > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = d / rho[:, None]
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    return np.array([total(t, dir_ok) for t in (x * x, x * y, x * z, y * y, y * z, z * z, x * r, y * r, z * r)] + [total(r * r, keep)])


def normal3(g):
    return np.array([[g[0], g[1], g[2]], [g[1], g[3], g[4]], [g[2], g[4], g[5]]]), np.array(g[6:9])


def _step(b, states, c, R, total=exact_sum, alter=None, seen=None):
    """(delta [3] or None, g [10]) of one Gauss-Newton step at the centre c: the step sums, their 3 x 3 Cholesky solve."""
    g = step_sums(b, states, c, R, total)
    N, rhs = normal3(g if alter is None else alter(g))
    delta = cholesky_solve(N, rhs, PIVOT_MIN * float(np.max(np.diag(N))), seen)
    if delta is None or not np.all(np.isfinite(delta)):
        return None, g
    return delta, g


def gauss_newton_step(b, states, c, R, total=exact_sum, alter=None, seen=None):
    """(c_next [3] or None where the step is refused, g [10]: the step sums at c): one step exactly as fit_ball's loop body takes it.
    `alter`: a function of the ten sums whose result is solved in their place -- the mutants of tests/test_treadmill_cases_host.py,
    which say what a comparison can and cannot see; `seen`: cholesky_solve's."""
    delta, g = _step(b, states, np.asarray(c, dtype=np.float64), float(R), total, alter, seen)
    return (None if delta is None else c + delta), g


def start_below(s, R):
    """m + m (R / |m|) of the 17 sums: the start of a known-radius fit that has no algebraic centre, or None where it has none either."""
    n = s[0]
    m = s[1:4] / n if n >= 3.0 else np.full(3, NAN)
    length = math.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) if n >= 3.0 else NAN
    if not (length > 0.0 and np.isfinite(length)):
        return None
    f = R / length
    return m + m * f


def fit_ball(b, states, radius=None, iterations=ITERATIONS, total=exact_sum, alter=None, seen=None):
    """dict(center [3], radius, rms, count, status, sums [17], steps: the lengths of the Gauss-Newton steps, last: the sums of the last
    step).  `alter`, `seen`: gauss_newton_step's; `seen` takes the algebraic fit's pivots first."""
    s = ball_sums(b, states, total)
    n = s[0]
    out = dict(center=np.full(3, NAN), radius=NAN, rms=NAN, count=int(n), status=REFUSED, sums=s, steps=[], last=None)
    fit = _algebraic(s, seen)
    status = 0
    if radius is None:
        if fit is None:
            return out
        c, R = fit
    else:
        R = float(radius)
        if fit is not None:
            c = fit[0]
        else:
            c = start_below(s, R)
            if c is None:
                return out
            status = START_BELOW
        for _ in range(iterations):
            delta, g = _step(b, states, c, R, total, alter, seen)
            if delta is None:
                out["status"] = status | REFUSED
                return out
            c = c + delta
            out["steps"].append(float(np.sqrt(delta @ delta)))
            out["last"] = g
    out.update(center=c, radius=R, rms=math.sqrt(step_sums(b, states, c, R, total)[9] / n), status=status)
    return out


def _solve_bar(A, Aabs, rhsabs, x, terms, absolute=0.0):
    """The standard perturbation bound of a linear system, ||dx|| <= ||A^-1|| (||db|| + ||dA|| ||x||) / (1 - ||A^-1|| ||dA||), with
    ||dA|| <= g ||Aabs||_F and ||db|| <= g ||rhsabs||, g = (terms + 64) u: an entry is a sum of `terms` products, in any order off by
    at most (terms - 1) u times the sum of their magnitudes (Aabs, rhsabs hold those), each product itself carries at most eight
    roundings (the subtraction of the centre, the squares and the sum of |q|^2, the product), and the Cholesky solve is backward
    stable with a constant below 32 u for a system of at most four unknowns (Higham, Accuracy and Stability, theorem 10.4: (3 n + 1) u
    per entry, twice for the two triangular solves): well below 64 u together.  `absolute`: what ||db|| carries on top, for a right
    side whose terms are not known to a relative error.  ||A^-1|| = cond(A) / ||A|| in the 2-norm, from the oracle's own matrix."""
    g = (terms + 64.0) * U
    inverse = float(np.linalg.cond(A) / np.linalg.norm(A, 2))
    dA, db = g * float(np.linalg.norm(Aabs)), g * float(np.linalg.norm(rhsabs)) + absolute
    assert inverse * dA < 0.5, "the matrix is too close to singular for a first-order bound"
    return inverse * (db + dA * float(np.linalg.norm(x))) / (1.0 - inverse * dA)


def ball_bar(b, states, fit):
    """(bar on |centre - oracle's|, bar on |radius - oracle's|) of an accepted algebraic fit `fit` (fit_ball's dict).  The system is
    A p = rhs with p = (2 a, k); _solve_bar bounds |dp|.  The centre is a + m: |dc| <= |dp| / 2 + 4 u |c| (the halving is exact; m's
    own error only moves the centring point, and the exact solution a + m does not depend on where the coordinates are centred).
    The radius is sqrt(k + |a|^2): |dR| <= (|dk| + 2 |a| |da|) / (2 R) + 4 u R."""
    s = fit["sums"]
    keep = samples(b, states).reshape(-1)
    m = s[1:4] / s[0]
    q = np.abs(np.asarray(b, dtype=np.float64).reshape(-1, 3)[keep] - m)
    g = np.concatenate([q, np.ones((len(q), 1))], axis=1)
    w = _dot(q, q)
    A, rhs = normal4(s)
    p = np.linalg.solve(A, rhs)
    dp = _solve_bar(A, g.T @ g, g.T @ w, p, len(q))
    c, R = fit["center"], fit["radius"]
    a = c - m
    return 0.5 * dp + 4.0 * U * float(np.linalg.norm(c)), (dp + 2.0 * float(np.linalg.norm(a)) * 0.5 * dp) / (2.0 * R) + 4.0 * U * R


def known_radius_bar(b, states, fit):
    """The bar on |centre - oracle's| of an accepted known-radius fit.  One Gauss-Newton step solves N delta = g with N = sum u u^T and
    g = sum u r; from the same centre, the device's step differs from the oracle's by at most e = _solve_bar(N, sum |u||u|^T, sum |u||r|,
    delta) -- where the residual r = rho - R is a difference of two numbers near R, known to 8 u rho (the subtraction of the centre, the
    three squares, two sums and the root behind rho, and the difference), not to a relative error: sum |u| 8 u rho joins ||dg|| -- and
    the update c + delta rounds by u |c| more.  The step map contracts towards its fixed point at a rate rho, which the oracle measures
    on its own steps and asserts to be at most 1/2; a sequence that errs by e per step then stays within e / (1 - rho) <= 2 e of the exact sequence, and both are within
    |last step| / (1 - rho) of their limit.  Bar: 2 e for the device, 2 e for the oracle's own sums were they rounded (they are exact),
    and 2 |last step| for what is left of the iteration: 4 e + 2 |last step| at the last step's matrix."""
    steps = fit["steps"]
    # the rate is that near the limit: a first step from far away obeys no rate, and below 1e-9 a step is rounding
    big = [k for k in range(1, len(steps)) if 1e-9 < steps[k - 1] <= 1e-2 * fit["radius"]]
    assert all(steps[k] <= 0.5 * steps[k - 1] for k in big), steps
    c = fit["center"]
    e = _step_solve_bar(b, states, c, fit["radius"], fit["last"], None)
    e += U * float(np.linalg.norm(c))
    return 4.0 * e + 2.0 * steps[-1]


def _step_solve_bar(b, states, c, R, g, terms):
    """_solve_bar on the 3 x 3 system of the step sums g, with the magnitudes sum |u||u|^T, sum |u||r| taken at the centre c and the
    residual's absolute error sum |u| 8 u rho on the right side (known_radius_bar).  `terms`: the summed terms of an entry, None for
    the sample count."""
    keep = samples(b, states).reshape(-1)
    d = np.asarray(b, dtype=np.float64).reshape(-1, 3)[keep] - c
    rho = np.sqrt(_dot(d, d))
    u, r = np.abs(d / rho[:, None]), np.abs(rho - R)
    N, rhs = normal3(g)
    return _solve_bar(N, u.T @ u, u.T @ r, np.linalg.solve(N, rhs), len(d) if terms is None else terms,
                      8.0 * U * float(np.linalg.norm(u.T @ rho)))


def step_bar(b, states, c, R):
    """The bar on |device's c_next - gauss_newton_step's c_next| where both step from the same centre c.  Derived, not measured: the
    device's delta solves the system of its own sums, n samples an entry in the kernel's order: within _solve_bar(terms = n) of the
    exact step (the residual's 8 u rho on the right side, as in known_radius_bar); the oracle's sums are exact (math.fsum), so its
    delta carries the roundings of the terms and of the solve alone: _solve_bar(terms = 0); and c + delta rounds once in each of
    the two, by at most u |c_next| per vector: 2 u (|c| + |delta|).  No contraction enters: one step, not a sequence."""
    c = np.asarray(c, dtype=np.float64)
    g = step_sums(b, states, c, R)
    N, rhs = normal3(g)
    delta = np.linalg.solve(N, rhs)
    e = _step_solve_bar(b, states, c, R, g, None) + _step_solve_bar(b, states, c, R, g, 0)
    return e + 2.0 * U * (float(np.linalg.norm(c)) + float(np.linalg.norm(delta)))


def rms_bar(b, states, fit, center_bar, radius_bar):
    """The bar on |rms - oracle's|.  rms is the root mean square of |b - c| - R: moving the centre by d moves every |b - c| by at most
    |d|, the radius moves every residual by its own error, and a residual is known to 8 u rho (known_radius_bar); the root mean square
    of numbers that each move by at most e moves by at most e.  The sum of n squares and the root add (n + 4) u rms."""
    keep = samples(b, states).reshape(-1)
    d = np.asarray(b, dtype=np.float64).reshape(-1, 3)[keep] - fit["center"]
    reach = float(np.sqrt(_dot(d, d)).max())
    return center_bar + radius_bar + 8.0 * U * reach + (fit["count"] + 4.0) * U * fit["rms"]


# ------------------------------------------------------------------------------------------------------------------ stage 3: the rotation
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def rotation_system(b, v, states, c):
    """(use [T, 6], M [T, 3, 3], rhs [T, 3], Mabs, rhsabs): sum (|r|^2 I - r r^T) and sum r x v over the legs in leg order, and the sums
    of the magnitudes of their terms."""
    use = samples(b, states) & np.all(np.isfinite(v), axis=-1)
    T = len(use)
    M, rhs, Mabs, rhsabs = np.zeros((T, 3, 3)), np.zeros((T, 3)), np.zeros((T, 3, 3)), np.zeros((T, 3))
    eye = np.eye(3)
    for leg in range(6):
        k = use[:, leg]
        r = np.where(k[:, None], b[:, leg], 0.0) - np.where(k[:, None], c, 0.0)
        vel = np.where(k[:, None], v[:, leg], 0.0)
        rr = _dot(r, r)
        for i in range(3):
            for j in range(3):
                term = (rr - r[:, i] * r[:, j]) if i == j else -(r[:, i] * r[:, j])
                M[:, i, j] = M[:, i, j] + np.where(k, term, 0.0)
        Mabs += rr[:, None, None] * eye + np.abs(r)[:, :, None] * np.abs(r)[:, None, :]
        rhs = rhs + _cross(r, vel)
        rhsabs += np.stack([np.abs(r[:, 1] * vel[:, 2]) + np.abs(r[:, 2] * vel[:, 1]), np.abs(r[:, 2] * vel[:, 0]) + np.abs(r[:, 0] * vel[:, 2]),
                            np.abs(r[:, 0] * vel[:, 1]) + np.abs(r[:, 1] * vel[:, 0])], axis=-1)
    return use, M, rhs, Mabs, rhsabs


def solve3(M, rhs, floor):
    """The Cholesky solve of solve3 in csrc/treadmill.hip on arrays: (w [T, 3], ok [T])."""
    with np.errstate(invalid="ignore", divide="ignore"):
        xx, xy, xz, yy, yz, zz = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
        ok = xx > floor
        l00 = np.sqrt(xx)
        l10, l20 = xy / l00, xz / l00
        d1 = yy - l10 * l10
        ok &= d1 > floor
        l11 = np.sqrt(d1)
        l21 = (yz - l20 * l10) / l11
        d2 = zz - l20 * l20 - l21 * l21
        ok &= d2 > floor
        l22 = np.sqrt(d2)
        y0 = rhs[:, 0] / l00
        y1 = (rhs[:, 1] - l10 * y0) / l11
        y2 = (rhs[:, 2] - l20 * y0 - l21 * y1) / l22
        wz = y2 / l22
        wy = (y1 - l21 * wz) / l11
        wx = (y0 - l10 * wy - l20 * wz) / l00
    w = np.stack([wx, wy, wz], axis=-1)
    ok &= np.all(np.isfinite(w), axis=-1)
    w[~ok] = np.nan
    return w, ok


def solve3_pivots(M):
    """[T, 3]: the three pivots solve3 compares with its floor, in its order (NaN after a pivot that is not positive)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        xx, xy, xz, yy, yz, zz = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
        l00 = np.sqrt(xx)
        l10, l20 = xy / l00, xz / l00
        d1 = yy - l10 * l10
        l21 = (yz - l20 * l10) / np.sqrt(d1)
        d2 = zz - l20 * l20 - l21 * l21
    return np.stack([xx, d1, d2], axis=-1)


def fictive_of(omega, c, R):
    """[..., 3] = (forward, sideways, yaw rate): u = -c / |c| (the body's origin is 0 in body coordinates), s = -(omega x R u)."""
    length = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    u = -c / length
    s = _cross(omega, np.broadcast_to(R * u, omega.shape))
    out = np.stack([-s[..., 0], -s[..., 1], -(omega[..., 0] * u[0] + omega[..., 1] * u[1] + omega[..., 2] * u[2])], axis=-1)
    return out if length > 0.0 else np.full(omega.shape, np.nan)


def ball_rotation(b, v, states, c, R, min_legs=MIN_LEGS):
    """dict(rotation [T, 3], legs [T] int32, residual [T], fictive [T, 3], bar [T]: the bar on |rotation - oracle's|, fictive_bar [T],
    residual_bar [T])."""
    b, v, c = np.asarray(b, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(c, dtype=np.float64)
    T = len(b)
    use, M, rhs, Mabs, rhsabs = rotation_system(b, v, states, c)
    legs = use.sum(axis=1).astype(np.int32)
    ball_ok = bool(np.all(np.isfinite(c)) and np.isfinite(R))
    w, ok = solve3(M, rhs, FRAME_PIVOT_MIN * (M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]))
    ok &= (legs >= min_legs) & ball_ok
    w[~ok] = np.nan
    sq, reach, speed = np.zeros(T), np.zeros(T), np.zeros(T)
    with np.errstate(invalid="ignore"):
        for leg in range(6):
            k = use[:, leg] & ok
            r = np.where(k[:, None], b[:, leg] - c, 0.0)
            e = np.where(k[:, None], v[:, leg], 0.0) - _cross(np.where(k[:, None], w, 0.0), r)
            sq = sq + np.where(k, _dot(e, e), 0.0)
            reach = np.maximum(reach, np.sqrt(_dot(r, r)))
            speed = np.maximum(speed, np.where(k, np.sqrt(_dot(v[:, leg], v[:, leg])), 0.0))
        residual = np.where(ok, np.sqrt(sq / legs.astype(np.float64)), np.nan)
        fictive = fictive_of(w, c, R) if ball_ok else np.full((T, 3), np.nan)
    fictive[~ok] = np.nan
    norm = np.sqrt(_dot(w, w))
    bar = np.full(T, np.nan)
    if ok.any():   # _solve_bar on every accepted frame at once: six terms per entry
        g = (6.0 + 64.0) * U
        inverse = np.linalg.cond(M[ok]) / np.linalg.norm(M[ok], 2, axis=(1, 2))
        dM, drhs = g * np.linalg.norm(Mabs[ok], axis=(1, 2)), g * np.linalg.norm(rhsabs[ok], axis=1)
        assert np.all(inverse * dM < 0.5), "a frame's matrix is too close to singular for a first-order bound"
        bar[ok] = inverse * (drhs + dM * norm[ok]) / (1.0 - inverse * dM)
    # fictive is linear in omega with |R u| = R: |d| <= R |d omega| and 8 u of its own roundings; the yaw rate likewise with |u| = 1.
    # residual = the root mean square of v - omega x r: it moves by at most max |r| |d omega|, and its own roundings are below 16 u
    # of the magnitudes that enter it
    fictive_bar = max(R, 1.0) * bar + 8.0 * U * max(R, 1.0) * norm if ball_ok else bar
    residual_bar = reach * bar + 16.0 * U * (speed + norm * reach)
    return dict(rotation=w, legs=legs, residual=residual, fictive=fictive, bar=bar, fictive_bar=fictive_bar, residual_bar=residual_bar)


# ------------------------------------------------------------------------------------------------------------------ stage 4: the path
def fictive_path(fictive, fps):
    """dict(path [T, 3] = (x, y, theta), skipped, theta_bar [T], xy_bar [T]): the recurrences themselves, frame after frame.
    theta_bar = (t + 2) u sum_{s<t} |yaw_s / fps|: a sum of t terms in any order is off by at most (t - 1) u times the sum of their
    magnitudes, and a term carries its division's u.  xy_bar = (t + 8) u sum_{s<t} (|forward_s| + |sideways_s|) / fps, the same with a
    term's roundings (sine and cosine at 2 u, two products, a sum, a division), plus sum_{s<t} theta_bar_s hypot(forward_s,
    sideways_s) / fps: a rotation by an angle off by d moves a vector of length l by at most d l."""
    f = np.asarray(fictive, dtype=np.float64)
    T = len(f)
    moves = np.all(np.isfinite(f), axis=1)
    path = np.zeros((T, 3))
    x = y = theta = 0.0
    a_theta = a_xy = turn = 0.0
    theta_bar, xy_bar = np.zeros(T), np.zeros(T)
    for t in range(T):
        path[t] = x, y, theta
        theta_bar[t] = (t + 2.0) * U * a_theta
        xy_bar[t] = (t + 8.0) * U * a_xy + turn
        if moves[t]:
            fw, sd, yaw = f[t].tolist()
            cs, sn = math.cos(theta), math.sin(theta)
            x = x + (cs * fw - sn * sd) / fps
            y = y + (sn * fw + cs * sd) / fps
            theta = theta + yaw / fps
            a_theta += abs(yaw / fps)
            a_xy += (abs(fw) + abs(sd)) / fps
            turn += theta_bar[t] * math.hypot(fw, sd) / fps
    return dict(path=path, skipped=int(T - moves.sum()), theta_bar=theta_bar, xy_bar=xy_bar)


def treadmill(X, fps, F, medians, states=None, radius=None, w=HALF, min_legs=MIN_LEGS, iterations=ITERATIONS):
    """The whole chain, a dict."""
    b, v = body_tips(X, fps, F, medians, w)
    if states is None:
        states = go.states_of(v[..., 0])
    fit = fit_ball(b, states, radius, iterations)
    rot = ball_rotation(b, v, states, fit["center"], fit["radius"], min_legs)
    return dict(tip=b, vel=v, states=states, fit=fit, **rot, **fictive_path(rot["fictive"], fps))


# ------------------------------------------------------------------------------------------------------------------ test inputs
def random_states(T, seed=0):
    """[T, 6] int32 in {-1, 0, 1}: frames of 0, 1, 2 and 6 stance legs among random ones."""
    rng = np.random.default_rng(seed)
    states = rng.choice(np.array([-1, 0, 0, 1], dtype=np.int32), size=(T, 6))
    for k, t in enumerate(range(0, T, 7)):
        count = (0, 1, 2, 6)[k % 4]
        states[t] = 1
        states[t, rng.permutation(6)[:count]] = 0
    return states.astype(np.int32)


def rotation_about(axis, angle):
    """[..., 3, 3]: Rodrigues' rotation about the unit vector `axis` by `angle` [...]."""
    a = np.asarray(axis, dtype=np.float64)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    angle = np.asarray(angle, dtype=np.float64)[..., None, None]
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


PLANTED = dict(T=600, fps=100.0, cycle=20, swing=4, radius=5.0, rate=4.09, depth=0.8)


def planted_ball(median_pose, kind="walk"):
    """dict(X [T, 38, 3], F, medians, center, radius, omega, states): `median_pose` [38, 3] in every frame, every tip on a sphere of
    radius PLANTED["radius"] whose centre lies beyond the tips' mean as seen from the body's origin, in body coordinates.  "walk":
    the ball turns at PLANTED["rate"] rad/s about the axis that carries its top backwards along ex; a leg in stance rides on it for
    cycle - swing frames and returns over the sphere, four times as fast, in `swing` frames, the two tripods half a cycle apart (gait
    oracle's walker on a ball).  "yaw": the ball turns about the axis through the fly, one full turn in T frames, and every leg rides
    on it throughout.  `states`: stance where the whole velocity window of a frame lies inside the leg's stance and the recording,
    swing elsewhere -- the frames whose central difference is a chord of the pure rotation."""
    P = PLANTED
    pose = np.asarray(median_pose, dtype=np.float64)
    F = jo.body_frame(pose)
    medians = pose[COXAE]
    o = origin(medians)
    rest = in_frame(pose[TIPS] - o, F)
    m = rest.mean(axis=0)
    R = P["radius"]
    c = m + P["depth"] * R * m / np.linalg.norm(m)
    u = -c / np.linalg.norm(c)
    ex = np.array([1.0, 0.0, 0.0])
    T, fps, n, swing = P["T"], P["fps"], P["cycle"], P["swing"]
    t = np.arange(T)
    on_ball = c + R * (rest - c) / np.linalg.norm(rest - c, axis=1)[:, None]
    tips = np.zeros((T, 6, 3))
    states = np.ones((T, 6), dtype=np.int32)
    w = HALF
    inside = (t >= w) & (t <= T - 1 - w)
    if kind == "walk":
        axis = np.cross(ex, u) / np.linalg.norm(np.cross(ex, u))   # s = R u x omega: along ex, forward
        omega = P["rate"] * axis
        step = P["rate"] / fps
        for leg, offset in enumerate(go.planted_offsets()):
            pos = np.mod(t - offset, n)   # 0 .. swing: the return; swing .. n: stance
            stance_angle = step * (pos - swing)
            angle = np.where(pos >= swing, stance_angle, step * (n - swing) * (1.0 - pos / swing))
            angle = angle - step * (n - swing) / 2.0   # the stance is centred on the resting tip
            tips[:, leg] = c + np.einsum("tij,j->ti", rotation_about(axis, angle), on_ball[leg] - c)
            states[(pos >= swing + w) & (pos <= n - 1 - w) & inside, leg] = 0
    else:
        omega = (2.0 * np.pi * fps / T) * u
        for leg in range(6):
            tips[:, leg] = c + np.einsum("tij,j->ti", rotation_about(u, 2.0 * np.pi * t / T), on_ball[leg] - c)
        states[inside] = 0
    X = np.repeat(pose[None], T, axis=0)
    X[:, TIPS] = o + tips @ F   # F^T b: the frame is orthonormal to rounding
    return dict(X=X, F=F, medians=medians, center=c, radius=R, omega=omega, states=states)


def chord_bound(rate, fps, w=HALF):
    """(|omega| w / fps)^2 / 6: the relative error of the central difference over +-w frames of a point on a circle -- a chord of half
    angle a = |omega| w / fps has length 2 sin(a) against the arc's 2 a, and sin(a) / a = 1 - a^2 / 6 + ..."""
    return (rate * w / fps) ** 2 / 6.0


def check_planted(r, planted, kind="walk", rounding=1e-9):
    """The planted ball's properties on one analysis r (the oracle's dict, or a device's result turned into one), computed with the
    planted states."""
    P = PLANTED
    T, fps = P["T"], P["fps"]
    c, R, omega = planted["center"], planted["radius"], planted["omega"]
    fit = r["fit"]
    assert fit["status"] == 0 and fit["count"] == int((planted["states"] == 0).sum())
    assert np.linalg.norm(fit["center"] - c) <= rounding and abs(fit["radius"] - R) <= rounding and fit["rms"] <= rounding
    rate = float(np.linalg.norm(omega))
    bound = chord_bound(rate, fps) + rounding
    moving = np.all(np.isfinite(r["rotation"]), axis=1)
    assert moving.sum() == (r["legs"] >= MIN_LEGS).sum() >= T - 2 * HALF - 2
    worst = float(np.max(np.linalg.norm(r["rotation"][moving] - omega, axis=1))) / rate
    assert worst <= bound, (worst, bound)
    want = fictive_of(omega, c, R)
    path = r["path"]
    frames = int(moving[:T - 1].sum())   # the path is an exclusive sum: the last frame's motion is not in it
    if kind == "walk":
        speed = float(np.hypot(want[0], want[1]))
        assert abs(want[2]) <= 1e-12 * rate   # no turning
        assert 0.9 * rate * R <= want[0] <= speed <= rate * R * (1.0 + 1e-12)   # forward, at the speed of the ball's top
        length = speed * frames / fps
        end = path[-1, :2]
        assert abs(np.linalg.norm(end) - length) <= bound * length, (np.linalg.norm(end), length)
        along = end / np.linalg.norm(end)
        off_line = np.abs(path[:, 0] * along[1] - path[:, 1] * along[0])
        assert off_line.max() <= bound * length and np.abs(path[:, 2]).max() <= bound * rate * T / fps
        assert np.all(np.diff(path[:, :2] @ along) >= 0.0)
    else:
        full = -2.0 * np.pi * frames / T   # the fly turns against the ball: a full turn, but for the frames that move nothing
        assert frames >= T - 2 * HALF - 2 and abs(path[-1, 2] - full) <= bound * 2.0 * np.pi, (path[-1, 2], full)
        assert np.abs(path[:, :2]).max() <= bound * R
    return worst, bound
