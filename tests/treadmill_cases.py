"""Seeded inputs for the sweep of the treadmill fit (csrc/treadmill.hip, DESIGN.md section 21, "swept"): the families of
tests/test_gpu_treadmill_sweep.py as tips b [T, 6, 3] and states [T, 6] handed in directly (fit_ball takes tips, so no pose is needed),
the rotation's and the path's inputs, the three-chunk inputs of the blocked scans, and the pivot decisions of a fit (pivot_decisions),
which tests/test_treadmill_cases_host.py certifies to be firm.  Host numpy only, seeded, every array read only.
TEST INFRASTRUCTURE ONLY."""
import collections
import functools

import numpy as np

import treadmill_oracle as to

CENTER, RADIUS = np.array([0.4, -0.3, -4.5]), 3.0      # the planted sphere of tests/test_gpu_treadmill.py
PLANE = 2.0                                             # the flat sets lie in the plane z = CENTER z + PLANE: a circle of the sphere
FPS = 100.0
CHUNK = to.B                                            # the frames behind one chunk of 256 block results: 65 536
T3 = 2 * CHUNK + 1                                      # 131 073: the first size whose carry is used a second time
# the same flags with 300 frames in the third chunk.  At T3 the third chunk is the recording's last frame, and no output of fill_gaps
# at a recording's last frame depends on the last good frame before it (nothing follows to interpolate towards): a carry of
# repair_scan_carry_kernel that forgot the first chunk would change nothing there.  From two frames in the third chunk on it does.
T3_FILL = 2 * CHUNK + 300

Case = collections.namedtuple("Case", "b states radius")   # radius: the known radius the family is fitted with (and None: free)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _case(b, states, radius=RADIUS):
    b, states = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(states, dtype=np.int32)
    assert b.shape == states.shape + (3,) and states.shape[1] == 6
    _frozen(b, states)
    return Case(b, states, float(radius))


def on_sphere(rng, shape, center=CENTER, radius=RADIUS):
    """Points of the planted sphere's cap that faces the body's origin (tests/test_gpu_treadmill.py's cap)."""
    d = rng.normal(size=tuple(shape) + (3,)) + np.array([0.0, 0.0, 2.0])
    return center + radius * d / np.linalg.norm(d, axis=-1, keepdims=True)


def on_circle(rng, shape, noise=0.0):
    """Points of the circle in which the planted sphere cuts the plane z = CENTER z + PLANE, moved out of the plane by N(0, noise)."""
    d = rng.normal(size=tuple(shape) + (2,))
    out = np.empty(tuple(shape) + (3,))
    out[..., :2] = CENTER[:2] + np.sqrt(RADIUS ** 2 - PLANE ** 2) * d / np.linalg.norm(d, axis=-1, keepdims=True)
    out[..., 2] = CENTER[2] + PLANE
    if noise:
        out[..., 2] += rng.normal(0.0, noise, size=tuple(shape))
    return out


def _filler(rng, T):
    """(b, states) without a sample: swing tips, unknown tips, and stance tips that are NaN, inf or NaN in one coordinate only."""
    b = on_sphere(rng, (T, 6))
    states = np.array([1, -1, 0, 1, 0, -1], dtype=np.int32)[(np.arange(T)[:, None] + np.arange(6)[None]) % 6].copy()
    bad = states == 0
    fill = np.array([np.nan, np.inf, -np.inf])
    k = 0
    for t, leg in zip(*np.nonzero(bad)):
        if k % 2:
            b[t, leg] = fill[k % 3]
        else:
            b[t, leg, k % 3] = fill[(k // 2) % 3]
        k += 1
    return b, states


def _place(rng, T, points, where):
    """The samples `points` [n, 3] at the (frame, leg) pairs `where`, every other lane a filler."""
    b, states = _filler(rng, T)
    for p, (t, leg) in zip(points, where):
        b[t, leg], states[t, leg] = p, 0
    assert int(to.samples(b, states).sum()) == len(points)
    return b, states


COUNTS = tuple(f"n{n}" for n in range(1, 6)) + ("spread3", "spread4", "spread5")
DEGENERATE = ("colinear3", "zero_mean3", "coplanar4", "identical8", "plane40_1e-7", "plane40_1e-3")
FAR_START = ("radius2", "radius6", "flat_circle")
FAMILIES = {"counts": COUNTS, "degenerate": DEGENERATE, "far_start": FAR_START}


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """A Case of the families `counts`, `degenerate` and `far_start`.
    n1 .. n5        n samples exactly on the planted sphere in the first n legs of one frame, the other legs fillers
    spread3 .. 5    the same n samples one per frame over T = 5, in a leg of their own each, among fillers
    colinear3       three samples on a line that misses the body's origin: no algebraic fit (n = 3), and from the start beyond their
                    mean the three directions lie in one plane: the first step is refused (status 3)
    zero_mean3      three samples of dyadic coordinates whose sum is exactly (0, 0, 0) in any order: no start either (status 1)
    coplanar4       four samples of a tilted plane's circle on the sphere: the 4 x 4 matrix is singular, the 3 x 3 step is not
    identical8      eight samples at one point: the 4 x 4 fit fails at its first pivot, the step at its second (status 3)
    plane40_<s>     40 samples of the flat circle, out of the plane by N(0, s): refused at 1e-7 (and fitted from below with the known
                    radius), accepted at 1e-3
    radius2, 6      48 samples on the planted sphere (R = 3) fitted with the radii 2 and 6: the algebraic centre is far from either fit
    flat_circle     tests/test_gpu_treadmill.py's flat circle under random states at T = 700: about 1 900 samples in three sum slices,
                    started beyond their mean"""
    rng = np.random.default_rng([21, sorted(sum(FAMILIES.values(), ())).index(name)])
    if name[0] == "n" and name[1:].isdigit():
        n = int(name[1:])
        return _case(*_place(rng, 1, on_sphere(rng, (n,)), [(0, leg) for leg in range(n)]))
    if name.startswith("spread"):
        n = int(name[6:])
        return _case(*_place(rng, 5, on_sphere(rng, (n,)), [(t, (2 * t + 1) % 6) for t in range(n)]))
    if name == "colinear3":
        a, d = np.array([1.0, -0.5, -2.0]), np.array([0.3, 0.9, 0.2])
        return _case(*_place(rng, 2, [a - d, a + 0.25 * d, a + 1.5 * d], [(0, 1), (0, 4), (1, 2)]))
    if name == "zero_mean3":
        p, q = np.array([1.5, -0.25, 2.0]), np.array([-0.75, 1.0, -3.5])
        return _case(*_place(rng, 1, [p, q, -(p + q)], [(0, 0), (0, 3), (0, 5)]))
    if name == "coplanar4":
        # the circle in which the sphere cuts the plane through CENTER + 2 n with the normal n
        n = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
        e1 = np.cross(n, [1.0, 0.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(n, e1)
        phi = np.array([0.3, 1.9, 3.2, 5.1])
        pts = CENTER + PLANE * n + np.sqrt(RADIUS ** 2 - PLANE ** 2) * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
        return _case(*_place(rng, 2, pts, [(0, 0), (0, 2), (1, 1), (1, 5)]))
    if name == "identical8":
        return _case(*_place(rng, 2, np.repeat(on_sphere(rng, (1,)), 8, axis=0), [(0, 0), (0, 1), (0, 3), (0, 4), (1, 0), (1, 2), (1, 3), (1, 5)]))
    if name.startswith("plane40_"):
        pts = on_circle(rng, (40,), float(name[8:]))
        return _case(*_place(rng, 12, pts, [(k % 12, (k // 12 + k) % 6) for k in range(40)]))
    if name in ("radius2", "radius6"):
        pts = on_sphere(np.random.default_rng([21, 99]), (48,))   # the same samples for both radii
        b, states = _place(np.random.default_rng([21, 98]), 20, pts, [(k % 20, (k // 20 + 2 * k) % 6) for k in range(48)])
        return _case(b, states, 2.0 if name == "radius2" else 6.0)
    if name == "flat_circle":
        T = 700
        return _case(on_circle(rng, (T, 6)), to.random_states(T, seed=T))
    raise KeyError(name)


def pivot_decisions(case, radius, total=to.exact_sum, iterations=to.ITERATIONS):
    """[(pivot, floor)] of every Cholesky pivot the fit of `case` with `radius` (None: free) compares, in order."""
    seen = []
    fit = to.fit_ball(case.b, case.states, radius, iterations, total, seen=seen)
    return seen, fit


# ------------------------------------------------------------------------------------------------------------------ the rotation
ROTATION_BALLS = {"planted": (*CENTER, RADIUS), "origin": (0.0, 0.0, 0.0, RADIUS), "nan_radius": (*CENTER, np.nan), "inf_radius": (*CENTER, np.inf)}
ROTATION_FRAMES = dict(parallel=12, velocity_nan=13)


@functools.lru_cache(maxsize=None)
def rotation_case():
    """(b [T, 6, 3], v [T, 6, 3], states [T, 6], usable [T]): frame t < 12 holds t % 6 + 1 usable legs -- for every min_legs in 2 .. 6 a
    frame of min_legs - 1, of min_legs and of 6 -- among legs in swing, unknown legs and stance legs whose tip is NaN; frame 12: three
    stance legs whose radii from CENTER are parallel (the spin about them is free: a refused pivot); frame 13: three stance legs, one
    with a NaN in its velocity alone (two usable); frames 14 .. 19: six stance legs, finite."""
    rng = np.random.default_rng([21, 7])
    T = 20
    b = on_sphere(rng, (T, 6)) + rng.normal(0.0, 0.02, (T, 6, 3))
    omega = np.array([0.7, -2.0, 0.4])
    v = np.cross(omega, b - CENTER) + rng.normal(0.0, 0.05, (T, 6, 3))
    states = np.zeros((T, 6), dtype=np.int32)
    usable = np.full(T, 6)
    for t in range(12):
        n = t % 6 + 1
        order = rng.permutation(6)
        for k, leg in enumerate(order[n:]):
            if (t + k) % 3 == 0:
                states[t, leg] = 1
            elif (t + k) % 3 == 1:
                states[t, leg] = -1
            else:
                b[t, leg, k % 3] = np.nan
        usable[t] = n
    t = ROTATION_FRAMES["parallel"]
    states[t, 3:] = 1
    b[t, 1] = CENTER + 0.5 * (b[t, 0] - CENTER)
    b[t, 2] = CENTER - 1.25 * (b[t, 0] - CENTER)
    usable[t] = 3
    t = ROTATION_FRAMES["velocity_nan"]
    states[t, 3:] = -1
    v[t, 1, 2] = np.nan
    usable[t] = 2
    return _frozen(b, v, states, usable)


# ------------------------------------------------------------------------------------------------------------------ the path
PATHS = ("edges", "large_yaw", "T65535", "T65536", "T131073", "carry3")
PATH_EDGE_RUNS = ((0, 3), (250, 256), (512, 520), (760, 775), (1024, 1280))


def _walk(rng, T):
    """Fictive motion of a plausible size: mm/s, mm/s, rad/s."""
    return rng.normal(0.0, 1.0, (T, 3)) * np.array([20.0, 5.0, 3.0])


@functools.lru_cache(maxsize=None)
def path_case(name):
    """fictive [T, 3], read only.
    edges       T = 1 537: non-finite runs over the frames PATH_EDGE_RUNS -- the first three frames, a run that ends on a scan block's
                last frame, one that starts on a block's first, one that spans an edge, a whole block --, NaN and +-inf by turns, and
                an infinity in one component only at frames 300, 301 and 302 (a component each)
    large_yaw   T = 512, a yaw of 2e4 rad/s at 100 fps: theta reaches 1e5 and the sine and cosine reduce large arguments
    T<n>        random motion with one frame in 97 non-finite
    carry3      T = 131 073: motion in the first 65 536 frames and in the last frame only: the second chunk of block results adds
                nothing, and the third chunk's only entry is what the carry still holds of the first"""
    rng = np.random.default_rng([21, 11, PATHS.index(name)])
    if name == "edges":
        f = _walk(rng, 1537)
        for k, (a, b) in enumerate(PATH_EDGE_RUNS):
            f[a:b] = (np.nan, np.inf, -np.inf)[k % 3]
        for c in range(3):
            f[300 + c, c] = np.inf if c % 2 else -np.inf
    elif name == "large_yaw":
        f = _walk(rng, 512)
        f[:, 2] = 2e4
    elif name == "carry3":
        f = np.zeros((T3, 3))
        f[:CHUNK] = _walk(rng, CHUNK)
        f[T3 - 1] = (7.0, -3.0, 1.0)
    else:
        T = int(name[1:])
        f = _walk(rng, T)
        f[::97, rng.integers(0, 3, size=len(f[::97]))] = np.nan
    return _frozen(f)


# ------------------------------------------------------------------------------------------------------------------ three chunks of carry
GAIT_DECISIVE = ((0, 0, "swing"), (1, 255, "stance"), (2, 256, "swing"), (3, 12345, "nan"), (4, 40000, "stance"), (5, CHUNK - 1, "swing"))


@functools.lru_cache(maxsize=None)
def gait_carry_velocity(on, off):
    """vel [T3, 6, 3]: the anterior velocity lies strictly between `off` and `on` -- it decides nothing -- but for one sample per leg in
    the first chunk (GAIT_DECISIVE: leg, frame, what it decides).  Every later state is that sample's, through two more chunks."""
    assert off < on
    rng = np.random.default_rng([21, 13])
    vel = rng.normal(0.0, 1.0, (T3, 6, 3))
    vel[..., 0] = off + (on - off) * rng.uniform(0.25, 0.75, (T3, 6))
    for leg, t, what in GAIT_DECISIVE:
        vel[t, leg, 0] = {"swing": on + 1.0, "stance": off - 1.0, "nan": np.nan}[what]
    return _frozen(vel)


FILL_JOINTS = dict(ends=3, first_chunk=11, last_chunk=22, middle=30)


@functools.lru_cache(maxsize=None)
def fill_carry_flags(T):
    """flags [T, 38] uint8 for T3 and T3_FILL, hand-made on four joints, the other 34 good throughout.  Joint `ends`: good at frames 0
    and T - 1 alone; `first_chunk`: good in frames 100 .. 199 and at 65 535 alone; `last_chunk`: good from frame 131 072 on alone (at
    T3 that is the last frame); `middle`: good at frames 0, 70 000 .. 70 009 and T - 1 alone.  The bad frames take the flags 1, 2
    and 3 by turns."""
    assert T in (T3, T3_FILL)
    bad = (1 + np.arange(T) % 3).astype(np.uint8)
    flags = np.zeros((T, 38), dtype=np.uint8)
    good = {k: np.zeros(T, bool) for k in FILL_JOINTS}
    good["ends"][[0, T - 1]] = True
    good["first_chunk"][100:200] = True
    good["first_chunk"][CHUNK - 1] = True
    good["last_chunk"][2 * CHUNK:] = True
    good["middle"][[0, T - 1]] = True
    good["middle"][70000:70010] = True
    for k, j in FILL_JOINTS.items():
        flags[:, j] = np.where(good[k], 0, bad)
    return _frozen(flags)


@functools.lru_cache(maxsize=None)
def fill_carry_points():
    """X [T3_FILL, 38, 3]: a random walk without a missing joint; the case at T3 takes its first T3 frames."""
    rng = np.random.default_rng([21, 17])
    X = rng.normal(0.0, 1.0, (1, 38, 3)) + np.cumsum(rng.normal(0.0, 0.01, (T3_FILL, 38, 3)), axis=0)
    return _frozen(X)
