"""A residual dial for the robust-loss bundle adjustment ("Sweep"): a BA problem in which every residual is a
number the test chose, exact to the bit, so that df3d_robust::row() can be probed at chosen z = (f / C)^2 through the real kernel.
Host numpy only.  TEST INFRASTRUCTURE ONLY.

The problem: two cameras with rotation vector 0 and translation 0 (cam_prep's first-order branch: R = I exactly), fx = fy = 1,
cx = cy = 0, every 3-D point at (0, 0, 1), seen by both cameras.  Then xc = yc = 0, iz = 1 and
    res = fx xc iz + cx - o = 0 - o = -o
under any contraction, so a detection of -f plants the residual f.  A detection of 0 means "unseen", so f = 0 comes from a point at
(1, 1, 1) with the detection (1, 1): 1 * 1 * 1 + 0 - 1 = +0.  (-0 cannot come out of that expression in round-to-nearest -- x - x is +0
and (-0) - o needs o = +0 = unseen; the cost kernel, which takes its residuals as they are, is fed -0 directly.)
What it reads out: a00 = a11 = 1 and the mixed terms are +-0, so the Jp planes (0, 0) and (1, 1) and the Jc translation planes (0, 3)
and (1, 4) hold s of the row itself, the w plane rho', the f plane f w / s.

Observations come in (frame, joint, camera) order, two residuals (x, y) each: point k owns the residual slots 4 k .. 4 k + 3.

tests/test_ba_robust_dial_host.py checks on the CPU, with the oracle and 50-digit mpmath alone, what the device tests rely on."""
import functools

import numpy as np

import ba_robust_oracle as bro

EPS = bro.EPS
F_SCALES = (0.5, 1.0, 5.0)             # C = 1 makes q = f exact
NOBS = (2, 254, 256, 258)              # the 256-lane block of ba_eval_robust_kernel: the exact multiple, both neighbours, and the smallest
K_ONE, K_ARCTAN = 32, 64               # f = C moved by -32 .. 32 ulp; f = C 3^(-1/4) moved by -64 .. 64 ulp
ARCTAN_Z0 = 3.0 ** -0.5                # 1 - 3 z^2 = 0
SPECIAL_EXPONENTS = (-600, -30, 10, 100, 250)     # z underflows to 0 ... arctan's t * t overflows while the row's values stay finite
FILL_SEED = 73


def _ulps(x, ks):
    """The positive float64 x moved by k representable numbers, for every k (k applications of nextafter: across a power of two the
    step halves, as the numbers do)."""
    return (np.array(x, np.float64).view(np.int64) + np.asarray(ks, np.int64)).view(np.float64)


def ladder_s2():
    """|s^2| targets from the clamp outwards through (EPS, 1e-6): two next to EPS, then 1, 2, 5 per decade."""
    return np.concatenate([EPS * np.array([1.5, 3.0]), (np.array([1.0, 2.0, 5.0])[None, :] * 10.0 ** np.arange(-15, -6)[:, None]).ravel()])


@functools.lru_cache(maxsize=None)
def values(C):
    """The dial values of f_scale C: dict(f=(n,) float64, group=(n,) '<U8', k=(n,) int).  group: 'one' (f = C moved by k ulp), 'arctan'
    (f = C 3^(-1/4) moved by k ulp), 'lad_c' / 'lad_a' (the ladders: cauchy's and arctan's s^2 stepping through +-(EPS, 1e-6); k is the
    ladder's index, negative on the clamped side), 'special' (C 2^k).  Both signs of every value: the negative ones follow in the same order."""
    f, group, k = [], [], []

    def add(vals, name, ks):
        f.extend(np.asarray(vals, np.float64).tolist())
        group.extend([name] * len(vals))
        k.extend(int(v) for v in ks)

    ks = np.arange(-K_ONE, K_ONE + 1)
    add(_ulps(np.float64(C), ks), "one", ks)
    ks = np.arange(-K_ARCTAN, K_ARCTAN + 1)
    add(_ulps(np.float64(C * 3.0 ** -0.25), ks), "arctan", ks)
    lad = ladder_s2()
    idx = np.arange(1, lad.size + 1)
    # cauchy: s^2 = (1 - z) / (1 + z)^2 ~ (1 - z) / 4 next to z = 1
    add(C * np.sqrt(1.0 - 4.0 * lad), "lad_c", idx)
    add(C * np.sqrt(1.0 + 4.0 * lad), "lad_c", -idx)
    # arctan: s^2 = (1 - 3 z^2) / (1 + z^2)^2 ~ -(27 / 8) z0 (z - z0) next to z0 = 3^(-1/2)
    dz = lad / (27.0 / 8.0 * ARCTAN_Z0)
    add(C * np.sqrt(ARCTAN_Z0 - dz), "lad_a", idx)
    add(C * np.sqrt(ARCTAN_Z0 + dz), "lad_a", -idx)
    add([C * 2.0**e for e in SPECIAL_EXPONENTS], "special", SPECIAL_EXPONENTS)
    f, group, k = np.array(f), np.array(group), np.array(k)
    assert np.isfinite(f).all() and (f > 0).all()
    return dict(f=np.concatenate([f, -f]), group=np.concatenate([group, group]), k=np.concatenate([k, k]))


@functools.lru_cache(maxsize=None)
def problems(C):
    """The dial's problems for f_scale C, one per entry of NOBS: a list of dict(nobs, npts, px (2, 1, npts, 2), intr (2, 3, 3), x (n,),
    planted (2 nobs,) -- the residual every slot has to come out as, to the bit --, dial (2 nobs,) bool: a dial value (not fill, not 0),
    zero (2 nobs,) bool: the slots of the f = 0 point).
    The dial values are dealt round-robin over the three large problems; the two-observation one takes four of them again; the rest of
    each problem is seeded normal fill of scale C."""
    v = values(C)["f"]
    rng = np.random.default_rng(FILL_SEED)
    big = [n for n in NOBS if n > 2]
    deal = {n: v[i :: len(big)] for i, n in enumerate(big)}
    deal[2] = np.array([C, -C * 3.0**-0.25, C * 2.0**100, -C * 2.0**-600])
    out = []
    for nobs in NOBS:
        m, npts = 2 * nobs, nobs // 2
        planted, dial, zero = rng.normal(0.0, C, m), np.zeros(m, bool), np.zeros(m, bool)
        mine = deal[nobs]
        room = m - (4 if nobs > 2 else 0)
        assert mine.size <= room, (nobs, mine.size, room)
        slots = np.sort(rng.choice(room, size=mine.size, replace=False))       # scattered among the fill, in the list's order
        planted[slots], dial[slots] = mine, True
        pts = np.tile([0.0, 0.0, 1.0], (npts, 1))
        obs = -planted.reshape(npts, 2, 2)                                     # [point, camera, (x, y)]
        if nobs > 2:                                                           # the last point: f = +0 four times
            planted[-4:], zero[-4:], dial[-4:] = 0.0, True, False
            pts[-1], obs[-1] = 1.0, 1.0
        assert (obs != 0).all(), "a detection of 0 means unseen"
        px = np.empty((2, 1, npts, 2))
        px[:, 0, :, 1] = obs[:, :, 0].T                                        # col = x
        px[:, 0, :, 0] = obs[:, :, 1].T                                        # row = y
        intr = np.tile(np.eye(3), (2, 1, 1))
        out.append(dict(nobs=nobs, npts=npts, px=px, intr=intr, x=np.concatenate([np.zeros(12), pts.ravel()]), planted=planted, dial=dial, zero=zero))
    assert sum(int(p["dial"].sum()) for p in out) == v.size + 4
    return out


def all_planted(C):
    """Every residual the dial plants for C (dial values, fill and zeros of all problems), in problem order."""
    return np.concatenate([p["planted"] for p in problems(C)])


def oracle_rows(loss, f, C):
    """The oracle's w, s, scaled f and clamped mask on the residuals f (overflow in t * t is part of what is probed: no warnings)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        z, w, s, clamped = bro.row_scale(loss, f, C)
        return z, w, s, f * w / s, clamped


# ---- 50-digit references ------------------------------------------------------------------------------------------------------------------
def mp_z(f, C):
    """(f / C)^2 in 50-digit arithmetic."""
    import mpmath as mp

    with mp.workdps(50):
        return (mp.mpf(float(f)) / mp.mpf(float(C))) ** 2


def mp_row(loss, f, C):
    """(w, s^2) of one residual in 50-digit arithmetic at the EXACT z = (f / C)^2 (huber: s^2 = 1 up to z = 1, 0 beyond, scipy's value
    without its rounding noise)."""
    import mpmath as mp

    with mp.workdps(50):
        z = (mp.mpf(float(f)) / mp.mpf(float(C))) ** 2
        if loss == "linear":
            return mp.mpf(1), mp.mpf(1)
        if loss == "soft_l1":
            return 1 / mp.sqrt(1 + z), (1 + z) ** mp.mpf(-1.5)
        if loss == "huber":
            return (mp.mpf(1), mp.mpf(1)) if z <= 1 else (1 / mp.sqrt(z), mp.mpf(0))
        if loss == "cauchy":
            return 1 / (1 + z), (1 - z) / (1 + z) ** 2
        if loss == "arctan":
            return 1 / (1 + z * z), (1 - 3 * z * z) / (1 + z * z) ** 2
    raise ValueError(loss)


def mp_rho(loss, z):
    """rho at the float64 z in 50-digit arithmetic (an mpf)."""
    import mpmath as mp

    with mp.workdps(50):
        z = mp.mpf(float(z))
        if loss == "linear":
            return +z
        if loss == "soft_l1":
            return 2 * (mp.sqrt(1 + z) - 1)
        if loss == "huber":
            return +z if z <= 1 else 2 * mp.sqrt(z) - 1
        if loss == "cauchy":
            return mp.log1p(z)
        if loss == "arctan":
            return mp.atan(z)
    raise ValueError(loss)


def rho_probe(C):
    """The subset of the dial that the one-rho-at-a-time test feeds df3d_ba_robust_cost with m = 1: z = 1 and its neighbours, arctan's
    zero, the ladders' ends, every special value, both zeros, one negative value of each kind."""
    v = values(C)
    f, g, k = v["f"], v["group"], v["k"]
    pick = ((g == "one") & np.isin(k, (-32, -2, -1, 0, 1, 2, 32))) | ((g == "arctan") & np.isin(k, (-64, -1, 0, 1, 64))) | (g == "special")
    pick |= np.isin(g, ("lad_c", "lad_a")) & np.isin(np.abs(k), (1, 15, 29))
    pos = pick & (f > 0)
    neg = pick & (f < 0) & (np.isin(g, ("special",)) | (k == 0))
    return np.concatenate([f[pos], f[neg], [0.0, -0.0]])
