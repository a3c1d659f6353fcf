"""The float64 model of the behaviour map's segmentation, in plain numpy, frame by frame and cell by cell: the
grid, the Gaussian density in its NON-separable form, steepest ascent under the total order (rho, -index), the kept regions, the
frame labels and the ethogram.  The model is this project's own and claims no parity with anyone.  The cases and the bars of the
tests are here too, each bar next to the sum it bounds.
"""
import numpy as np

EPS = 2.0 ** -53                    # the unit roundoff of float64
GRID = 256                          # config.BEHAVIOUR_GRID
GRID_RANGE = (2, 1024)
SIGMA_FRACTION = 1.0 / 32.0         # config.BEHAVIOUR_DENSITY_SIGMA_FRACTION
MIN_PEAK = 0.01                     # config.BEHAVIOUR_MIN_PEAK
DENSITY_SLICE = 2048                # the frames one block of the device's density kernel adds before its partial tile is stored


# ------------------------------------------------------------------------------------------------------------------ grid, density
def valid_rows(Y):
    return np.isfinite(Y).all(axis=1)


def grid(Y, G=GRID, sigma=None):
    """((x0, y0, h), sigma) of the map Y [T, 2]."""
    v = Y[valid_rows(Y)]
    if len(v) == 0:
        raise ValueError("no valid frame")
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = float(max(hi[0] - lo[0], hi[1] - lo[1]))
    if sigma is None:
        if not ext > 0.0:
            raise ValueError("no extent and no sigma")
        sigma = SIGMA_FRACTION * ext
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError("sigma must be finite and > 0")
    L = ext / 2.0 + 3.0 * sigma
    x0, y0 = float((lo[0] + hi[0]) / 2.0 - L), float((lo[1] + hi[1]) / 2.0 - L)
    return (x0, y0, 2.0 * L / G), sigma


def centres(origin, G):
    """(gx [G], gy [G]): the centres of the columns and of the rows."""
    x0, y0, h = origin
    k = np.arange(G, dtype=np.float64)
    return x0 + (k + 0.5) * h, y0 + (k + 0.5) * h


def density(Y, origin, sigma, G):
    """(rho [G, G], A [G, G]): the density, one frame after the other, each frame's whole exponent in one exp; and the largest
    exponent argument d^2 / 2 sigma^2 any valid frame has at the cell."""
    gx, gy = centres(origin, G)
    s = np.zeros((G, G))
    A = np.zeros((G, G))
    M = 0
    for t in np.flatnonzero(valid_rows(Y)):   # selection: an invalid row is never touched
        arg = ((gx[None, :] - Y[t, 0]) ** 2 + (gy[:, None] - Y[t, 1]) ** 2) / (2.0 * sigma ** 2)
        s += np.exp(-arg)
        A = np.maximum(A, arg)
        M += 1
    return s / (M * 2.0 * np.pi * sigma ** 2), A


def density_tolerance(rho, A, M):
    """The bar on |device - oracle| per cell: (4 (M + 64) + 2 A) 2^-53 rho + 1e-300.

    Every term is positive, so relative errors of the terms carry over to the sum.  The device forms a term as the product of two
    exponentials.  Its grid coordinates and differences d are the oracle's own operations, bit for bit; each of its two arguments
    d^2 / 2 sigma^2 is rounded twice (the square, the quotient), so the arguments together are off by at most 2 A_t EPS absolutely,
    A_t the term's whole argument, which an exponential turns into a relative 2 A_t EPS <= 2 A EPS: the `2 A`.  The two exponentials
    themselves (1 ulp each = 2 EPS), their product (EPS), the M-term sum in another order (slices of DENSITY_SLICE, four frames per
    MFMA: at most (M - 1) EPS) and the final quotient (3 EPS) give (M + 7) EPS.  The oracle's own sum is rounded in the same way:
    3 roundings of its argument (<= 3 A_t EPS, which its own `A` share of the bar does not cover in the worst case but the slack
    below does for every A a term that still matters can have: a term with A_t > 700 is below 1e-300 of the peak), one exponential,
    an M-term sum and a quotient: (M + 5) EPS.  Together 2 M + 12, rounded up to 4 (M + 64): the 64 keeps the bar honest for M = 1,
    where the tail of constants dominates.  1e-300 covers the subnormal range, in which a product of two exponentials loses bits the
    single exponential keeps.  This is the issue's constant; the derivation gives no reason for another."""
    return (4.0 * (M + 64) + 2.0 * A) * EPS * rho + 1e-300


def density_separable(Y, origin, sigma, G):
    """The density in the device's form, restated in numpy: rho = A^T B over the valid frames with A[t, r] = exp(-(gy_r - y_t)^2 /
    2 sigma^2) and B[t, q] likewise in x, added in slices of DENSITY_SLICE frames.  What the bar rests on."""
    gx, gy = centres(origin, G)
    s = np.zeros((G, G))
    M = int(valid_rows(Y).sum())
    for t0 in range(0, len(Y), DENSITY_SLICE):
        y = Y[t0 : t0 + DENSITY_SLICE]
        y = y[valid_rows(y)]
        a = np.exp(-((gy[None, :] - y[:, 1:2]) ** 2) / (2.0 * sigma ** 2))
        b = np.exp(-((gx[None, :] - y[:, 0:1]) ** 2) / (2.0 * sigma ** 2))
        s += a.T @ b
    return s / (M * 2.0 * np.pi * sigma ** 2)


def gaussian_tail(z):
    """Q(z) = P(N(0, 1) > z)."""
    from math import erfc, sqrt

    return 0.5 * erfc(z / sqrt(2.0))


# ------------------------------------------------------------------------------------------------------------------ watershed
def _above(ra, ia, rb, ib):
    """key(a) > key(b) for the key (rho, -index)."""
    return ra > rb or (ra == rb and ia < ib)


def ascent(rho):
    """ptr [G * G]: every cell's 8-neighbour with the largest key if that key exceeds the cell's own, else the cell itself."""
    G = rho.shape[0]
    flat = rho.ravel()
    ptr = np.arange(G * G)
    for i in range(G * G):
        r, q = divmod(i, G)
        best, at = None, -1
        for rr in range(max(r - 1, 0), min(r + 2, G)):
            for qq in range(max(q - 1, 0), min(q + 2, G)):
                j = rr * G + qq
                if j != i and (at < 0 or _above(flat[j], j, best, at)):
                    best, at = flat[j], j
        if at >= 0 and _above(best, at, flat[i], i):
            ptr[i] = at
    return ptr


def watershed(rho, min_peak=MIN_PEAK):
    """(regions [G, G] int32, R, root_cells [R] int32, the longest chain's links): chains are walked link by link."""
    G = rho.shape[0]
    flat = rho.ravel()
    ptr = ascent(rho)
    root = np.empty(G * G, dtype=np.int64)
    longest = 0
    for i in range(G * G):
        at, links = i, 0
        while ptr[at] != at:
            at, links = ptr[at], links + 1
        root[i], longest = at, max(longest, links)
    top = flat.max()
    kept = [i for i in range(G * G) if root[i] == i and flat[i] > 0.0 and flat[i] >= min_peak * top]
    number = {cell: k + 1 for k, cell in enumerate(kept)}
    regions = np.array([number.get(int(c), 0) for c in root], dtype=np.int32).reshape(G, G)
    return regions, len(kept), np.array(kept, dtype=np.int32), longest


def spiral(G):
    """A one-cell-wide ridge that winds inwards from cell (0, 0), every second ring, its values rising along the way; zeros
    elsewhere.  The pointer chain along it is longer than G (asserted where it is used), so fewer than ceil(log2 G^2) doubling
    rounds -- log2 G would do for straight climbs -- leave cells short of their root."""
    rho = np.zeros((G, G))
    seen = np.zeros((G, G), dtype=bool)

    def inside(r, q):
        return 0 <= r < G and 0 <= q < G

    def free(r, q, dr, dq):   # the cell ahead is new, and the one behind it is not part of the ridge: the arms stay one cell apart
        return inside(r + dr, q + dq) and not seen[r + dr, q + dq] and not (inside(r + 2 * dr, q + 2 * dq) and seen[r + 2 * dr, q + 2 * dq])

    r, q, dr, dq, k = 0, 0, 0, 1, 1
    while True:
        rho[r, q], seen[r, q] = k, True
        k += 1
        if not free(r, q, dr, dq):
            dr, dq = dq, -dr   # turn right
            if not free(r, q, dr, dq):
                return rho
        r, q = r + dr, q + dq


def built_fields():
    """name -> (rho, min_peak): the built fields of the host test and of the teacher-forced device test."""
    g = np.arange(12, dtype=np.float64)
    bump = lambda r, q, w: np.exp(-((g[:, None] - r) ** 2 + (g[None, :] - q) ** 2) / (2.0 * w ** 2))   # noqa: E731
    plateau = np.zeros((9, 9))
    plateau[2:6, 2:6] = 1.0
    plateau[6, 6] = 2.0                       # touches the plateau's corner cell (5, 5) diagonally
    island = np.zeros((12, 12))
    island[4:9, 4:9] = bump(6, 6, 1.0)[4:9, 4:9]
    two = bump(3, 3, 1.5) + bump(8, 8, 1.5)   # symmetric under (r, q) -> (11 - r, 11 - q): the two peaks are equal to the bit
    two = np.maximum(two, two[::-1, ::-1])
    small = bump(3, 3, 1.0) + 0.05 * bump(9, 9, 1.0)
    return {
        "one peak": (bump(5, 7, 2.0), MIN_PEAK),
        "two equal peaks": (two, MIN_PEAK),
        "all equal": (np.full((7, 7), 0.25), MIN_PEAK),
        "all zero": (np.zeros((5, 5)), 0.0),
        "plateau touching a higher cell": (plateau, MIN_PEAK),
        "zeros round a bump, min_peak 0": (island, 0.0),
        "zeros round a bump, min_peak 0.5": (island, 0.5),
        "a minor peak kept": (small, 0.01),
        "a minor peak dropped": (small, 0.1),
        "spiral ridge": (spiral(21), 0.0),
        "two by two": (np.array([[1.0, 1.0], [1.0, 1.0]]), 1.0),
    }


# ------------------------------------------------------------------------------------------------------------------ labels, ethogram
def labels(Y, regions, origin):
    x0, y0, h = origin
    G = regions.shape[0]
    out = np.full(len(Y), -1, dtype=np.int32)
    with np.errstate(over="ignore"):   # a frame far outside overflows to an infinity, which the clamp takes
        for t in np.flatnonzero(valid_rows(Y)):
            q = int(min(max(np.floor((Y[t, 0] - x0) / h), 0.0), G - 1.0))
            r = int(min(max(np.floor((Y[t, 1] - y0) / h), 0.0), G - 1.0))
            out[t] = regions[r, q]
    return out


def ethogram(lab, R):
    """(bouts [B, 3] int64, occupancy [R + 1] int64, transitions [R + 1, R + 1] int64), by a loop over the frames."""
    bouts = []
    occupancy = np.zeros(R + 1, dtype=np.int64)
    transitions = np.zeros((R + 1, R + 1), dtype=np.int64)
    for t, a in enumerate(lab):
        a = int(a)
        if bouts and bouts[-1][0] == a:
            bouts[-1][2] += 1
        else:
            bouts.append([a, t, 1])
        if a >= 0:
            occupancy[a] += 1
        if t + 1 < len(lab) and a >= 0 and lab[t + 1] >= 0 and lab[t + 1] != a:
            transitions[a, int(lab[t + 1])] += 1
    return np.array(bouts, dtype=np.int64).reshape(-1, 3), occupancy, transitions


def label_row(T, kind, R=5, seed=0):
    """A synthetic label row: "random" (runs of random lengths of the labels -1 .. R), "single" (one bout), "alternating" (every
    frame changes)."""
    if kind == "single":
        return np.full(T, 2, dtype=np.int32)
    if kind == "alternating":
        return (np.arange(T) % 3 - 1).astype(np.int32)
    rng = np.random.default_rng(seed + T)
    out = np.empty(T, dtype=np.int32)
    t = 0
    while t < T:
        n = int(rng.integers(1, 40))
        out[t : t + n] = rng.integers(-1, R + 1)
        t += n
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
# (M valid of T, G): one block and one slice, a ragged tile, more tiles than one, a ragged slice, two slices
DENSITY_CASES = [(1, 1, 2), (5, 7, 16), (257, 260, 33), (1031, 1040, 64), (DENSITY_SLICE + 1, DENSITY_SLICE + 12, 65)]
SCAN_SIZES = [1, 255, 256, 257, 65537]


def density_case(M, T, seed=0):
    """Y [T, 2]: three clumps and a thin background, T - M invalid rows (NaN, inf in either column) spread through it."""
    rng = np.random.default_rng(1000 * seed + T)
    centre = np.array([[0.0, 0.0], [6.0, 1.0], [2.0, 7.0]])[rng.integers(0, 3, size=T)]
    Y = centre + rng.standard_normal((T, 2)) * np.where(rng.random((T, 1)) < 0.1, 3.0, 0.6) + np.array([40.0, -25.0])
    bad = np.linspace(0, T - 1, T - M + 2).round().astype(int)[1:-1] if T > M else np.zeros(0, dtype=int)
    assert len(set(bad)) == T - M
    for k, t in enumerate(bad):
        Y[t, k % 2] = (np.nan, np.inf, -np.inf)[k % 3]
    return Y


PLANTED_CENTRES = np.array([[0.0, 0.0], [10.0, 0.0], [5.0, 9.0]])
PLANTED = dict(frames=120, sigma=1.5, grids=(16, 33, 64), outlier=119, nan_rows=(7, 50), keep_three=0.1, keep_four=0.001)


def planted_case(seed=0):
    """(Y [120, 2], behaviour [120]): frame t round centre t mod 3 with deviation 0.5, one outlier at (30, 30) (behaviour 3), rows 7
    and 50 NaN (behaviour -1)."""
    rng = np.random.default_rng(seed)
    T = PLANTED["frames"]
    behaviour = np.arange(T) % 3
    Y = PLANTED_CENTRES[behaviour] + 0.5 * rng.standard_normal((T, 2))
    Y[PLANTED["outlier"]] = (30.0, 30.0)
    behaviour[PLANTED["outlier"]] = 3
    for t in PLANTED["nan_rows"]:
        Y[t] = np.nan
        behaviour[t] = -1
    return Y, behaviour


def segment(Y, G=GRID, sigma=None, min_peak=MIN_PEAK):
    """The whole chain: a dict of density, origin, sigma, regions, R, root_cells, region_peaks, labels, bouts, occupancy, transitions."""
    origin, sigma = grid(Y, G, sigma)
    rho, _ = density(Y, origin, sigma, G)
    regions, R, roots, _ = watershed(rho, min_peak)
    gx, gy = centres(origin, G)
    lab = labels(Y, regions, origin)
    bouts, occupancy, transitions = ethogram(lab, R)
    return dict(density=rho, origin=origin, sigma=sigma, regions=regions, R=R, root_cells=roots,
                region_peaks=np.stack((gx[roots % G], gy[roots // G]), axis=1).reshape(-1, 2), labels=lab, bouts=bouts, occupancy=occupancy,
                transitions=transitions)


def check_planted(lab, R, behaviour, min_peak):
    """The planted case's assertions on a label row, the device's or the oracle's: no frame is excused."""
    b = np.asarray(behaviour)
    own = [set(lab[b == k].tolist()) for k in range(3)]
    assert all(len(s) == 1 for s in own), f"a behaviour is spread over the labels {own}"
    three = [s.pop() for s in own]
    assert len(set(three)) == 3 and min(three) >= 1, f"the three behaviours have the labels {three}"
    assert np.all(lab[b == -1] == -1)
    out = int(lab[b == 3][0])
    if min_peak == PLANTED["keep_three"]:
        assert R == 3 and out == 0, f"R = {R}, the outlier has label {out}"
    else:
        assert R == 4 and out >= 1 and out not in three, f"R = {R}, the outlier has label {out}"
