"""Float64 oracle of the t-SNE behaviour map: the model in plain numpy.  It is this project's own
specification -- it claims no parity with DeepFly3D, MotionMapper or scikit-learn -- and csrc/behaviour_map.hip is tested against
it.  The derived error bars of the GPU tests live here too, next to the sums they bound."""
import functools

import numpy as np

FLOOR = 1e-9
MAX_POINTS = 8192
POINTS_CAP = 16384
PERPLEXITY = 32.0
ENTROPY_TOL = 1e-10
BETA_MAX = 1e12
ITERATIONS = 1000
EXAGGERATION_ITERATIONS = 250
EPS = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------ rules 1 and 2
def distributions(S):
    """(p [T, D], valid [T]): rule 1.  Invalid rows are NaN."""
    S = np.asarray(S, dtype=np.float64)
    S = S.reshape(S.shape[0], -1)
    D = S.shape[1]
    with np.errstate(all="ignore"):
        a = S.sum(axis=1)
        valid = np.all(np.isfinite(S) & (S >= 0), axis=1) & np.isfinite(a) & (a > 0)
    p = np.full(S.shape, np.nan)
    p[valid] = (S[valid] / a[valid, None] + FLOOR) / (1.0 + D * FLOOR)
    return p, valid


def train_rows(valid_count, max_points=MAX_POINTS):
    """Rule 2: the positions of the training rows in the list of valid rows."""
    N = min(int(valid_count), int(max_points))
    return np.array([(i * int(valid_count)) // N for i in range(N)], dtype=np.int64)


def check_perplexity(u, n):
    if not (np.isfinite(u) and u > 1.0):
        raise ValueError("perplexity must be finite and > 1")
    if 3.0 * u > n:
        raise ValueError(f"perplexity {u:g} needs at least {int(np.ceil(3 * u))} admitted entries, the row has {n}")


# ------------------------------------------------------------------------------------------------------------------ rule 3
def divergence(pa, pb):
    """K [M, N] = max(0, sum_d pa[i, d] (log pa[i, d] - log pb[j, d])), every pair summed on its own (no cancellation of two
    large sums: the oracle is the more accurate side)."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    la, lb = np.log(pa), np.log(pb)
    K = np.empty((pa.shape[0], pb.shape[0]))
    for i in range(pa.shape[0]):
        K[i] = (pa[i][None, :] * (la[i][None, :] - lb)).sum(axis=1)
    return np.maximum(K, 0.0)


def divergence_tolerance(pa, pb, constant=4.0):
    """The bar per element of K = e_i - sum_d pa[i, d] log pb[j, d] as the kernel forms it.  e_i and the product are sums of D
    terms, each term a rounded product of a rounded logarithm (2 roundings), summed in some order: the error of each is at most
    (D + 2) 2^-53 times the sum of the terms' sizes (Higham, 'Accuracy and Stability', section 4.2, first order), and the final
    subtraction adds one rounding of a value no larger than either.  `constant` = 4 covers the two sums, the subtraction and the
    second-order terms: bar = 4 (D + 2) 2^-53 sum_d pa[i, d] (|log pa[i, d]| + |log pb[j, d]|)."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    D = pa.shape[1]
    size = (pa * np.abs(np.log(pa))).sum(axis=1)[:, None] + pa @ np.abs(np.log(pb)).T
    return constant * (D + 2) * EPS * size


# ------------------------------------------------------------------------------------------------------------------ rule 4
def entropy(k, beta):
    """(H, S, mean k, var k) of the admitted entries k (already minus their minimum) at beta."""
    w = np.exp(-beta * k)
    S = w.sum()
    q = (k * w).sum() / S
    var = (k * k * w).sum() / S - q * q
    return np.log(S) + beta * q, S, q, var


def calibrate_row(k, u):
    """(beta, info) of one row's admitted entries: bisection, geometric while the bracket spans more than a factor of two."""
    k = k - k.min()
    target = np.log(u)
    if entropy(k, BETA_MAX)[0] - target > ENTROPY_TOL:
        return BETA_MAX, 1
    lo, hi = 0.0, BETA_MAX
    beta = 1.0 / max(k.mean(), 1.0 / BETA_MAX)
    beta = min(beta, BETA_MAX)
    for _ in range(400):
        diff = entropy(k, beta)[0] - target
        if abs(diff) <= ENTROPY_TOL:
            return beta, 0
        if diff > 0:
            lo = beta
        else:
            hi = beta
        if lo == 0.0:
            beta = hi / 2.0
        elif hi > 2.0 * lo:
            beta = np.sqrt(lo * hi)
        else:
            beta = 0.5 * (lo + hi)
    raise AssertionError("the oracle's bisection did not meet the entropy rule")


def calibrate(K, u=PERPLEXITY, exclude=None):
    """(cond [M, N], beta [M], info [M]): rule 4.  exclude: None, "self" or an integer array [M] (-1: none)."""
    K = np.asarray(K, dtype=np.float64)
    M, N = K.shape
    if isinstance(exclude, str):
        exclude = np.arange(M)
    check_perplexity(u, N - (0 if exclude is None else 1))
    cond, beta, info = np.zeros((M, N)), np.empty(M), np.zeros(M, dtype=np.int32)
    for i in range(M):
        keep = np.ones(N, dtype=bool)
        if exclude is not None and exclude[i] >= 0:
            keep[exclude[i]] = False
        k = K[i, keep]
        beta[i], info[i] = calibrate_row(k, u)
        w = np.exp(-beta[i] * (k - k.min()))
        cond[i, keep] = w / w.sum()
    return cond, beta, info


def row_entropy(K_row, beta, exclude=-1):
    """(H, |dH/dbeta|, k - k_mean over the admitted entries, keep mask) of one row at a given beta."""
    keep = np.ones(K_row.shape[0], dtype=bool)
    if exclude >= 0:
        keep[exclude] = False
    k = K_row[keep] - K_row[keep].min()
    H, _, q, var = entropy(k, beta)
    return H, beta * var, k - q, keep


def conditional_tolerance(c, dk, slope, n):
    """The bar per admitted entry of a calibrated row c (the oracle's) against one calibrated on its own: both betas sit within
    bar_H = ENTROPY_TOL + entropy_rounding(n) of the target in H, so within 2 bar_H / |dH/dbeta| of each other (1 % for the
    curvature); dc_j / dbeta = c_j (k_mean - k_j); the weights' own rounding is a relative (n + 8) 2^-52.  `dk` and `slope` are
    row_entropy's."""
    bar_H = ENTROPY_TOL + entropy_rounding(n)
    return 1.01 * c * np.abs(dk) * 2.0 * bar_H / slope + 8.0 * (n + 8) * EPS * c


def entropy_rounding(n):
    """What rounding may add to an n-term evaluation of H = log S + beta Q / S: every weight carries the exponential's own error and
    the rounding of its argument (a relative beta k 2^-53, which sums to 2^-53 beta Q / S <= 2^-53 log n over the row), S and Q
    are n-term sums (relative (n + 2) 2^-53 each), and H <= log n.  With the constant 4 for the quotient, the logarithm and
    second order: 4 (n + 8) 2^-53 (1 + log n)."""
    return 4.0 * (n + 8) * EPS * (1.0 + np.log(n))


# ------------------------------------------------------------------------------------------------------------------ rules 5 and 6
def joint(cond):
    N = cond.shape[0]
    P = (cond + cond.T) / (2.0 * N)
    np.fill_diagonal(P, 0.0)
    return P


def schedule(k):
    return (12.0, 0.5) if k < EXAGGERATION_ITERATIONS else (1.0, 0.8)


def learning_rate(N):
    return max(N / 48.0, 50.0)


def pair_terms(Y):
    d = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (d * d).sum(axis=2))
    wz = w.copy()
    np.fill_diagonal(wz, 0.0)
    return d, w, wz.sum()


def gradient(P, Y, alpha=1.0):
    d, w, Z = pair_terms(Y)
    return 4.0 * (((alpha * P - w / Z) * w)[:, :, None] * d).sum(axis=1)


def gradient_tolerance(P, Y, alpha):
    """The bar per component of g_i = 4 (alpha sum_j P w d - sum_j w^2 d / Z).  Each of the N terms carries a handful of roundings
    (the difference, 1 + |d|^2, the reciprocal, two products), the sums add at most (N - 1) more in any order, and Z, a sum of
    positive terms, is off by a relative (N + 8) 2^-53 at the most, which the factor 2 on the second sum carries.  As in section
    16 the worst case of an N-term sum is taken, with a constant of 4: 4 (N + 64) 2^-53 * 4 (alpha sum_j P w |d| + 2 sum_j w^2 |d| / Z)."""
    d, w, Z = pair_terms(Y)
    N = Y.shape[0]
    size = 4.0 * ((alpha * P * w)[:, :, None] * np.abs(d)).sum(axis=1) + 8.0 * ((w * w)[:, :, None] * np.abs(d)).sum(axis=1) / Z
    return 4.0 * (N + 64) * EPS * size


def step(P, Y, V, G, k):
    """One iteration k: (Y, V, G, g) afterwards."""
    alpha, mu = schedule(k)
    g = gradient(P, Y, alpha)
    G = np.where(g * V < 0.0, G + 0.2, G * 0.8)
    G = np.maximum(G, 0.01)
    V = mu * V - learning_rate(Y.shape[0]) * G * g
    return Y + V, V, G, g


def run(P, Y0, n_iter=ITERATIONS, first_iter=0, state=None, keep=()):
    """(Y, V, G) after iterations first_iter .. first_iter + n_iter - 1; `keep`: iteration indices whose state BEFORE the step is
    returned as a dict {k: (Y, V, G)} in a fourth element."""
    Y = np.array(Y0, dtype=np.float64)
    V, G = (np.zeros_like(Y), np.ones_like(Y)) if state is None else (np.array(state[0]), np.array(state[1]))
    kept = {}
    for k in range(first_iter, first_iter + n_iter):
        if k in keep:
            kept[k] = (Y.copy(), V.copy(), G.copy())
        Y, V, G, _ = step(P, Y, V, G, k)
    return (Y, V, G, kept) if keep else (Y, V, G)


def cost(P, Y):
    _, w, Z = pair_terms(Y)
    m = P > 0
    return float((P[m] * np.log(P[m] * Z / w[m])).sum())


def cost_tolerance(P, Y):
    """The bar of the cost, an N^2-term sum of P (log P + log Z - log w): the worst case of the sum with the constant 4, as for the
    gradient."""
    _, w, Z = pair_terms(Y)
    m = P > 0
    return 4.0 * (Y.shape[0] + 64) * EPS * float((P[m] * (np.abs(np.log(P[m])) + abs(np.log(Z)) + np.abs(np.log(w[m])))).sum())


def initial(N, seed=0):
    import torch

    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return (1e-4 * torch.randn((N, 2), generator=gen, dtype=torch.float64)).numpy()


def perturbed(Y0, count=8, relative=1e-15, seed=99):
    rng = np.random.default_rng(seed)
    return [Y0 * (1.0 + relative * rng.choice([-1.0, 1.0], size=Y0.shape)) for _ in range(count)]


# ------------------------------------------------------------------------------------------------------------------ rule 7, the whole
def place(cond, Y):
    return cond @ Y


def behaviour_map(S, perplexity=PERPLEXITY, n_iter=ITERATIONS, max_points=MAX_POINTS, seed=0, Y0=None):
    """dict(embedding [T, 2], train_index [N], beta [T], info [T], kl, P, Y): the whole model."""
    if not 1 <= max_points <= POINTS_CAP:
        raise ValueError("max_points")
    p, valid = distributions(S)
    T = p.shape[0]
    vidx = np.flatnonzero(valid)
    rows = train_rows(len(vidx), max_points) if len(vidx) else np.zeros(0, dtype=np.int64)
    N = len(rows)
    check_perplexity(perplexity, N - 1)
    train = vidx[rows]
    cond, beta_t, info_t = calibrate(divergence(p[train], p[train]), perplexity, "self")
    P = joint(cond)
    Y = run(P, initial(N, seed) if Y0 is None else Y0, n_iter)[0]
    embedding, beta, info = np.full((T, 2), np.nan), np.full(T, np.nan), np.zeros(T, dtype=np.int32)
    embedding[train], beta[train], info[train] = Y, beta_t, info_t
    rest = np.setdiff1d(vidx, train)
    if len(rest):
        c, b, i = calibrate(divergence(p[rest], p[train]), perplexity)
        embedding[rest], beta[rest], info[rest] = place(c, Y), b, i
    return dict(embedding=embedding, train_index=train, beta=beta, info=info, kl=cost(P, Y), P=P, Y=Y)


# ------------------------------------------------------------------------------------------------------------------ shared cases
def spectra(T, D, seed, centres=3, spread=0.25, zeros=0.0):
    """[T, D] non-negative spectra drawn round `centres` centres, the labels interleaved in time; a fraction `zeros` of the entries
    is exactly zero (there the floor is what keeps the divergence finite)."""
    rng = np.random.default_rng(seed)
    base = rng.gamma(2.0, 1.0, size=(centres, D))
    label = np.arange(T) % centres
    S = base[label] * np.exp(spread * rng.standard_normal((T, D)))
    if zeros:
        S[rng.random((T, D)) < zeros] = 0.0
        S[:, 0] += 0.5   # no row becomes all zero
    return S, label


TEACHER_SIZES = (13, 64, 65, 257)
TEACHER_STAGES = (0, 120, 399)   # the start (all distances about 1e-4), mid-exaggeration, the end of a 400-iteration run


@functools.lru_cache(maxsize=None)
def teacher_case(N):
    """(P, {k: (Y, V, G) before iteration k}) of the teacher-forced tests: N spectra of 25 channels, perplexity 4 at N = 13 and 10
    above, the oracle run for 400 iterations from seed N."""
    S, _ = spectra(N, 25, seed=170 + N)
    p, _ = distributions(S)
    P = joint(calibrate(divergence(p, p), 4.0 if N == 13 else 10.0, "self")[0])
    kept = run(P, initial(N, seed=N), 400, keep=TEACHER_STAGES)[3]
    return P, kept


def step_comparison(P, state, k, got):
    """The oracle's step k from `state` against `got` = (Y, V, G): (worst fraction of the bar over Y, V and G, the fraction of
    components excused).  A component is excused where the oracle's own g V lies within the gradient's bar of zero (V != 0: a
    zero velocity gives an exact zero in both): there the gain may take either branch."""
    Y, V, G = state
    alpha, _ = schedule(k)
    Yn, Vn, Gn, g = step(P, Y, V, G, k)
    bar_g = gradient_tolerance(P, Y, alpha)
    excused = (V != 0.0) & (np.abs(g) <= bar_g)
    lr = learning_rate(Y.shape[0])
    bar_V = lr * Gn * bar_g + 4.0 * EPS * (np.abs(V) + lr * Gn * np.abs(g))
    bar_Y = bar_V + 2.0 * EPS * np.abs(Yn)
    ok = ~excused
    with np.errstate(all="ignore"):
        fy = np.where(ok, np.abs(got[0] - Yn) / bar_Y, 0.0).max()
        fv = np.where(ok, np.abs(got[1] - Vn) / bar_V, 0.0).max()
    fg = 0.0 if np.array_equal(np.asarray(got[2])[ok], Gn[ok]) else np.inf
    return max(fy, fv, fg), excused.mean()


LARGE_SIZES = (1024, 1025, 1283)   # one full trip of the gradient kernel's 1024-column loop; a second trip of one column; one of 259
LARGE_SYNTHETIC = {120: (5, 3.0), 399: (6, 20.0)}   # stage: (seed, scale) of the synthetic states
GAINS = (0.01, 0.64, 0.8, 1.0, 1.2, 2.4)


@functools.lru_cache(maxsize=None)
def large_cond(N):
    """cond [N, N] of N spectra of 25 channels at perplexity 10, the row itself excluded."""
    p = distributions(spectra(N, 25, seed=170 + N)[0])[0]
    return calibrate(divergence(p, p), 10.0, "self")[0]


def synthetic_state(N, seed, scale):
    """(Y, V, G) that no run has to reach: three clusters of spread 0.2 scale round centres drawn N(0, scale^2), frame t in
    cluster t mod 3, velocities N(0, (0.01 scale)^2) and gains from GAINS (the floor, both branches' products, the start)."""
    rng = np.random.default_rng(seed)
    centres = scale * rng.standard_normal((3, 2))
    Y = centres[np.arange(N) % 3] + 0.2 * scale * rng.standard_normal((N, 2))
    V = 0.01 * scale * rng.standard_normal((N, 2))
    G = rng.choice(np.array(GAINS), size=(N, 2))
    return Y, V, G


@functools.lru_cache(maxsize=None)
def large_case(N):
    """(P, {k: (Y, V, G) before iteration k}) for one teacher-forced step at the sizes of LARGE_SIZES.  The oracle is NOT run
    for 400 iterations here (minutes): stage 0 is the real start, stages 120 and 399 are synthetic_state's -- a state does not
    have to be reachable for one step from it to be checked."""
    P = joint(large_cond(N))
    Y0 = initial(N, seed=N)
    states = {0: (Y0, np.zeros_like(Y0), np.ones_like(Y0))}
    for k, (seed, scale) in LARGE_SYNTHETIC.items():
        states[k] = synthetic_state(N, seed, scale)
    assert sorted(states) == list(TEACHER_STAGES)
    return P, states


# the calibration keeps its row in 8 N bytes of dynamic LDS: the last size below 48 KiB and the first above it (there the launch
# raises the kernel's limit), both sides of 64 KiB (8192 is the default training size) and the cap
WIDE_SIZES = (6144, 6145, 8192, 8193, 16384)
WIDE_TIES = 40


@functools.lru_cache(maxsize=None)
def wide_case(N):
    """(pa [4, 25], pb [N, 25], K [5, N], exclude [5] int32): four ordinary rows of divergences against N columns and a fifth in
    which WIDE_TIES entries tie exactly at the row's minimum -- spread over the whole row, column N - 2 among them -- and every
    other entry lies at least 0.75 above: at the default perplexity of 32 that row cannot be calibrated.  `exclude` is the
    explicit list: the last column, none, the first, one in the 17th stride of a 256-thread loop, and for the tied row the
    column next to its last tie."""
    pa = distributions(spectra(4, 25, seed=N)[0])[0]
    pb = distributions(spectra(N, 25, seed=N + 1)[0])[0]
    K = np.empty((5, N))
    K[:4] = divergence(pa, pb)
    K[4] = np.abs(np.random.default_rng(N + 2).standard_normal(N)) + 1.0
    K[4, wide_ties(N)] = 0.25
    return pa, pb, K, np.array([N - 1, -1, 0, 4097, N - 1], dtype=np.int32)


def wide_ties(N):
    ties = np.unique(np.linspace(2, N - 2, WIDE_TIES).astype(np.int64))
    assert len(ties) == WIDE_TIES and ties[-1] == N - 2
    return ties


PLANTED = dict(D=40, spread=0.12, seed=1717, perplexity=10.0, n_iter=500, max_points=120, invalid=(6, 51, 112, 179))


@functools.lru_cache(maxsize=None)
def planted_spectra():
    """(S [184, D], labels [184] (-1: invalid)) of planted_case, without the oracle's runs."""
    c = PLANTED
    T = 180 + len(c["invalid"])
    full, lab = spectra(T, c["D"], c["seed"], spread=c["spread"])
    a, b, n, z = c["invalid"]
    full[a] = 0.0
    full[b, 3] = np.nan
    full[n] = -full[n]
    full[z, 5] = np.inf
    lab = lab.copy()
    lab[list(c["invalid"])] = -1
    assert [int((lab == k).sum()) for k in range(3)] == [60, 60, 60]
    return full, lab


@functools.lru_cache(maxsize=None)
def planted_case():
    """(S [184, D], labels [184] (-1: invalid), the oracle's result, the final KL of eight perturbed starts): three planted
    behaviours interleaved in time (frame t shows behaviour t mod 3), four invalid rows that leave 60 valid frames each.  120 of
    the 180 valid frames are embedded and 60 placed; the invalid rows shift the phase of the training rule floor(1.5 i) against
    the labels, so every behaviour has training frames and placed ones."""
    c = PLANTED
    full, lab = planted_spectra()
    res = behaviour_map(full, c["perplexity"], c["n_iter"], c["max_points"], seed=0)
    Y0 = initial(c["max_points"], 0)
    kls = [cost(res["P"], run(res["P"], y, c["n_iter"])[0]) for y in perturbed(Y0)]
    return full, lab, res, np.array(kls)


def separation(embedding, label):
    """(every valid frame's nearest neighbour carries its own label, the smallest between-label distance, the largest own-label
    nearest-neighbour distance)."""
    ok = label >= 0
    Y, lab = embedding[ok], label[ok]
    d = np.sqrt(((Y[:, None] - Y[None]) ** 2).sum(axis=2))
    np.fill_diagonal(d, np.inf)
    same = lab[:, None] == lab[None, :]
    own = np.where(same, d, np.inf).min(axis=1)
    other = np.where(~same, d, np.inf).min(axis=1)
    return bool(np.all(own < other)), float(other.min()), float(own.max())
