"""Float64 statement of the gait model in plain numpy: tip position and velocity in leg coordinates, swing and
stance by hysteresis -- a Python loop over time, the serial recurrence itself, so that the device's scan is tested against something
that is not a scan --, lift-offs, touch-downs and steps, the phase of every leg, the coupling of the six phases and the support
patterns.  The model is this project's own specification; it claims no parity with anything.  Also here: the bars of the three
floating-point comparisons with their derivations, the numpy restatement of the coupling kernel's form, and the planted walker."""
import math
import os

import numpy as np

import joint_angles_oracle as jo

HALF = 2                      # config.GAIT_DIFF_HALF
ON, OFF = 5.0, 0.0            # config.GAIT_SWING_ON, GAIT_SWING_OFF
TRIPODS = (21, 42)            # config.GAIT_TRIPODS: legs 0, 2, 4 and legs 1, 3, 5
SLICE, THREADS, WAVE = 2048, 256, 64   # constants of csrc/gait.hip: the frames of one coupling block, its lanes, a wave
U = 2.0 ** -53                # the unit round-off of float64
TWO_PI = 6.283185307179586476925286766559

TIPS = [jo.leg_joints(leg)[4] for leg in range(6)]
COXAE = [jo.leg_joints(leg)[0] for leg in range(6)]
SIGMA = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])


def missing(P):
    """[..., 3] -> [...]: section 14's rule, all three coordinates exactly 0 or any of them not finite."""
    P = np.asarray(P, dtype=np.float64)
    return np.all(P == 0.0, axis=-1) | ~np.all(np.isfinite(P), axis=-1)


def leg_coordinates(v, F):
    """q(v) of v [T, 6, 3] in the frames F [T, 3, 3]: (v . ex, sigma v . ey, v . ez), every dot product as x x + y y + z z from the
    left, one IEEE operation at a time (numpy's element-wise ufuncs never fuse)."""
    def dot(e):
        e = e[:, None, :]
        return v[..., 0] * e[..., 0] + v[..., 1] * e[..., 1] + v[..., 2] * e[..., 2]

    return np.stack([dot(F[:, 0]), SIGMA * dot(F[:, 1]), dot(F[:, 2])], axis=-1)


def window(T, w):
    """(a [T], b [T]): the clipped ends of the velocity's window."""
    t = np.arange(T)
    return np.maximum(t - w, 0), np.minimum(t + w, T - 1)


def tip_kinematics(X, fps, body_frame="recording", w=HALF):
    """X [T, 38, 3] -> (tip [T, 6, 3], vel [T, 6, 3])."""
    X = np.asarray(X, dtype=np.float64)
    T = len(X)
    if T == 0:
        return np.zeros((0, 6, 3)), np.zeros((0, 6, 3))
    F = np.ascontiguousarray(jo.frames_for(X, body_frame), dtype=np.float64)
    frame_ok = np.all(np.isfinite(F.reshape(T, 9)), axis=1)[:, None]
    a, b = window(T, w)
    P0, P4 = X[:, COXAE], X[:, TIPS]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tip = leg_coordinates(P4 - P0, F)
        scale = (fps / (b - a).astype(np.float64))[:, None, None]   # one division
        vel = leg_coordinates(P4[b] - P4[a], F) * scale
    tip[~(frame_ok & ~missing(P0) & ~missing(P4))] = np.nan
    vel[~(frame_ok & (b > a)[:, None] & ~missing(P4[a]) & ~missing(P4[b]))] = np.nan
    return tip, vel


def velocity_bar(X, fps, body_frame, w=HALF):
    """[T, 6, 3]: 8 u (fps / (b - a)) sum_k |F_rk| |d_k| with d = P4[b] - P4[a].  One evaluation of a component rounds every term of
    the dot product at most six times -- the subtraction that forms d_k, the product with F_rk, the two sums of the dot product
    (the last term meets only one), the division fps / (b - a) and the product with it; the mirror's factor of +-1 is exact -- so it
    lies within ((1 + u)^6 - 1) < 8 u of the exact value of sum_k |F_rk| |d_k| times the scale.  The kernel is built without
    contraction and performs the oracle's operations in the oracle's order, so the difference the test expects is zero; the bar is
    what a reordering of the three terms could cost."""
    X = np.asarray(X, dtype=np.float64)
    T = len(X)
    F = np.abs(np.ascontiguousarray(jo.frames_for(X, body_frame), dtype=np.float64))
    a, b = window(T, w)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = np.abs(X[b][:, TIPS] - X[a][:, TIPS])
        s = np.einsum("trk,tlk->tlr", F, d)
        return 8.0 * U * (fps / (b - a).astype(np.float64))[:, None, None] * s


def duration_bar(durations):
    """4 u |duration|.  The oracle divides, q = (t1 - t0) / fps: one rounding of the exact quotient e, |q - e| <= u |e|.  A device
    that multiplies by a reciprocal rounds 1 / fps and then the product: it lies within ((1 + u)^2 - 1) |e| of e.  The two differ by
    at most (3 u + u^2) |e| <= (3 u + u^2) (1 + u + u^2) |q| < 4 u |q|.  csrc/gait.hip divides like the oracle, so the difference the
    test measures is zero; the bar holds for either form."""
    return 4.0 * U * np.abs(durations)


def coupling_bar(count):
    """(n + 32) u per component of the mean.  The n terms have magnitude <= 1; their sum in any order is off by at most (n - 1) u
    times the sum of their magnitudes, <= n, so the mean by (n - 1) u; a term itself carries the rounding of 2 pi phase (<= 4 u
    at an angle below 2 pi), of the sine and cosine (1 u each) and, in the kernel's product form, of two products and a sum: well
    below 32 u together."""
    return (np.asarray(count, dtype=np.float64) + 32.0) * U


def states_of(u, on=ON, off=OFF):
    """u [T, 6] -> states [T, 6] int32, by the recurrence itself."""
    T = len(u)
    states = np.full((T, 6), -1, dtype=np.int32)
    for leg in range(6):
        s = -1
        column = u[:, leg].tolist()
        for t in range(T):
            x = column[t]
            if x != x:
                s = -1
            elif x > on:
                s = 1
            elif x < off:
                s = 0
            states[t, leg] = s
    return states


def events(states):
    """(lift [T, 6] bool, touch [T, 6] bool)."""
    s = np.asarray(states)
    lift, touch = np.zeros(s.shape, dtype=bool), np.zeros(s.shape, dtype=bool)
    lift[1:] = (s[:-1] == 0) & (s[1:] == 1)
    touch[1:] = (s[:-1] == 1) & (s[1:] == 0)
    return lift, touch


def steps_of(states, tip, fps):
    """(steps [S, 4] int64, metrics [S, 3])."""
    s = np.asarray(states)
    lift, touch = events(s)
    rows, metrics = [], []
    for leg in range(6):
        at = np.flatnonzero(lift[:, leg])
        for t0, t2 in zip(at[:-1], at[1:]):
            if np.any(s[t0:t2 + 1, leg] == -1):
                continue
            downs = np.flatnonzero(touch[t0:t2 + 1, leg]) + t0
            assert len(downs) == 1, "exactly one touch-down between two lift-offs"
            t1 = int(downs[0])
            rows.append((leg, int(t0), t1, int(t2)))
            with np.errstate(invalid="ignore"):
                metrics.append(((t1 - t0) / fps, (t2 - t1) / fps, tip[t1, leg, 0] - tip[t0, leg, 0]))
    return np.array(rows, dtype=np.int64).reshape(-1, 4), np.array(metrics, dtype=np.float64).reshape(-1, 3)


def phase_of(states):
    """[T, 6]: (t - t0) / (t2 - t0) inside a step, NaN outside."""
    s = np.asarray(states)
    phase = np.full(s.shape, np.nan)
    for leg, t0, _, t2 in steps_of(s, np.zeros(s.shape + (3,)), 1.0)[0]:
        phase[t0:t2, leg] = np.arange(0, t2 - t0, dtype=np.float64) / np.float64(t2 - t0)
    return phase


def coupling(phase):
    """(mean [6, 6, 2], count [6, 6] int64): the model's own form, cos and sin of the difference, summed exactly (math.fsum)."""
    p = np.asarray(phase, dtype=np.float64)
    mean, count = np.full((6, 6, 2), np.nan), np.zeros((6, 6), dtype=np.int64)
    ok = np.isfinite(p)
    for i in range(6):
        for j in range(6):
            both = ok[:, i] & ok[:, j]
            n = int(both.sum())
            count[i, j] = n
            if n:
                ang = TWO_PI * (p[both, i] - p[both, j])
                mean[i, j] = math.fsum(np.cos(ang)) / n, math.fsum(np.sin(ang)) / n
    return mean, count


def coupling_kernel_form(phase):
    """The same in the form and the order of gait_coupling_kernel: the six unit vectors of a frame once, cos(a - b) = ca cb + sa sb
    and sin(a - b) = sa cb - ca sb, a lane's eight frames of a slice in order, the shuffle tree over a wave, the four waves in
    order, the slices in order.  What remains between this and the device is the two libraries' sine and cosine."""
    p = np.asarray(phase, dtype=np.float64)
    T = len(p)
    slices = (T + SLICE - 1) // SLICE
    ok = np.zeros((slices * SLICE, 6), dtype=bool)
    ok[:T] = np.isfinite(p)
    ang = np.zeros((slices * SLICE, 6))
    ang[:T] = TWO_PI * np.where(ok[:T], p, 0.0)
    c, s = np.cos(ang), np.sin(ang)

    def block_sum(x):   # x [slices, SLICE]
        lanes = np.zeros((slices, THREADS))
        for k in range(SLICE // THREADS):
            lanes = lanes + x[:, k * THREADS:(k + 1) * THREADS]
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
        return out

    mean, count = np.full((6, 6, 2), np.nan), np.zeros((6, 6), dtype=np.int64)
    for i in range(6):
        for j in range(i, 6):
            both = ok[:, i] & ok[:, j]
            n = int(both.sum())
            count[i, j] = count[j, i] = n
            if n:
                re = block_sum(np.where(both, c[:, i] * c[:, j] + s[:, i] * s[:, j], 0.0).reshape(slices, SLICE))
                im = block_sum(np.where(both, s[:, i] * c[:, j] - c[:, i] * s[:, j], 0.0).reshape(slices, SLICE))
                mean[i, j] = re / n, im / n
                mean[j, i] = re / n, -im / n
    return mean, count


def patterns(states):
    """(pattern [T] int32, histogram [64] int64, state_counts [6, 3] int64)."""
    s = np.asarray(states)
    mask = ((s == 1).astype(np.int32) << np.arange(6, dtype=np.int32)).sum(axis=1).astype(np.int32)
    pattern = np.where(np.any(s == -1, axis=1), np.int32(-1), mask).astype(np.int32)
    histogram = np.bincount(pattern[pattern >= 0], minlength=64).astype(np.int64)
    counts = np.stack([(s == -1).sum(axis=0), (s == 0).sum(axis=0), (s == 1).sum(axis=0)], axis=1).astype(np.int64)
    return pattern, histogram, counts


def gait(X, fps, body_frame="recording", on=ON, off=OFF, w=HALF):
    """The whole chain, a dict."""
    tip, vel = tip_kinematics(X, fps, body_frame, w)
    states = states_of(vel[..., 0], on, off)
    steps, metrics = steps_of(states, tip, fps)
    phase = phase_of(states)
    mean, count = coupling(phase)
    pattern, histogram, counts = patterns(states)
    return dict(tip=tip, vel=vel, states=states, steps=steps, step_metrics=metrics, phase=phase, coupling=mean, coupling_count=count,
                pattern=pattern, pattern_histogram=histogram, state_counts=counts)


# ---------------------------------------------------------------------------------------------------------------------- test inputs
def u_cases(T, seed=0, block=THREADS):
    """u [T, 6] for the state rule: leg 0 random with long in-band runs that cross block edges; leg 1 the same with runs of NaN; leg 2
    in-band but for a decisive sample as the last lane of every other block and the first of the block after it; leg 3 never leaves
    the band; leg 4 alternates every frame; leg 5 mostly NaN."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(OFF, ON, size=(T, 6))   # in band: (OFF, ON) is open at ON, and OFF itself is in band too
    decisive = rng.random(T) < 0.02
    u[decisive, 0] = rng.choice([ON + 1.0, OFF - 1.0], size=int(decisive.sum()))
    u[:, 1] = u[:, 0]
    for start in rng.integers(0, max(T, 1), size=max(T // 300, 1)):
        u[start:start + int(rng.integers(1, 2 * block)), 1] = np.nan
    edge = np.arange(block - 1, T, 2 * block)
    u[edge, 2] = ON + 2.0
    u[edge[edge + 1 < T] + 1, 2] = OFF - 2.0
    u[::2, 4], u[1::2, 4] = ON + 1.0, OFF - 1.0
    u[:, 5] = np.where(rng.random(T) < 0.9, np.nan, rng.choice([ON + 1.0, OFF - 1.0, 2.0], size=T))
    if T > 3:
        u[T // 2, 0], u[T // 2 + 1, 0] = ON, OFF   # exactly on a threshold: in band
    return u


def random_poses(T, seed=0):
    """X [T, 38, 3]: a slow drift of every joint plus noise, with a few missing tips and coxae and one non-finite tip."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (1, 38, 3)) + 0.01 * np.cumsum(rng.normal(0.0, 1.0, (T, 38, 3)), axis=0) + rng.normal(0.0, 0.05, (T, 38, 3))
    if T > 6:
        X[rng.integers(0, T, size=max(T // 50, 2)), TIPS[1]] = 0.0
        X[rng.integers(0, T, size=max(T // 100, 1)), COXAE[4]] = 0.0
        X[T // 2, TIPS[3], 1] = np.inf
    return X


def random_frames(T, seed=0):
    """F [T, 3, 3]: one random rotation, tilted a little more in every frame (orthonormal to rounding, which the model does not ask for)."""
    rng = np.random.default_rng(seed)
    ang = 0.3 * np.cumsum(rng.normal(0.0, 0.01, T))
    c, s = np.cos(ang), np.sin(ang)
    tilt = np.zeros((T, 3, 3))
    tilt[:, 0, 0], tilt[:, 0, 1], tilt[:, 1, 0], tilt[:, 1, 1], tilt[:, 2, 2] = c, -s, s, c, 1.0
    return tilt @ jo.random_rotation(rng)


PLANTED = dict(T=600, fps=100.0, cycle=20, duty=0.4, speed=40.0, missing_leg=2, missing_frames=(310, 311))


def planted_offsets():
    """The frame of the cycle at which every leg lifts off: the tripod of legs 0, 2, 4 at 0, that of legs 1, 3, 5 half a cycle on."""
    return [0 if (TRIPODS[0] >> leg) & 1 else PLANTED["cycle"] // 2 for leg in range(6)]


def planted_sawtooth(c):
    """The tip's anterior position at cycle position c (any real): up at `speed` for `duty` of the cycle, back down over the rest."""
    n, fps = PLANTED["cycle"], PLANTED["fps"]
    swing = PLANTED["duty"] * n
    top = PLANTED["speed"] / fps * swing
    c = np.mod(c, n)
    return np.where(c <= swing, PLANTED["speed"] / fps * c, top - (c - swing) * top / (n - swing))


def planted_walker(median_pose):
    """X [T, 38, 3]: `median_pose` [38, 3] in every frame, every tip moved along the pose's own anterior axis by the sawtooth, the
    two tripods half a cycle apart, and the tip of one leg zeroed in two frames in the middle of one of its steps."""
    pose = np.asarray(median_pose, dtype=np.float64)
    ex = jo.body_frame(pose)[0]
    T = PLANTED["T"]
    X = np.repeat(pose[None], T, axis=0)
    t = np.arange(T)
    for leg, offset in enumerate(planted_offsets()):
        X[:, TIPS[leg]] = pose[TIPS[leg]] + planted_sawtooth(t - offset)[:, None] * ex
    X[list(PLANTED["missing_frames"]), TIPS[PLANTED["missing_leg"]]] = 0.0
    return X


def planted_shift(w=HALF, on=ON):
    """The frames by which the central difference over +-w frames moves a planted lift-off: with the sawtooth x = -down c before the
    lift-off at cycle position 0 and x = up c after it, the first c at which (x(c + w) - x(c - w)) fps / 2 w exceeds `on`.  (The
    stance before it is below `off`, so the state it leaves is stance; w is shorter than swing and stance.)"""
    n, fps = PLANTED["cycle"], PLANTED["fps"]
    swing = PLANTED["duty"] * n
    up = PLANTED["speed"] / fps
    down = up * swing / (n - swing)
    assert w < swing and w < n - swing

    def x(c):
        return up * c if c >= 0 else -down * c

    for c in range(-w, w + 1):
        if (x(c + w) - x(c - w)) * fps / (2 * w) > on:
            return c
    raise AssertionError("the window hides the lift-off")


def planted_lift_offs(w=HALF):
    """{leg: the frames t >= 1 at which the walker's leg is found to lift off}: every start of its cycle, moved by planted_shift.
    None of them lies within w frames of the recording's ends, where the window is clipped."""
    T, n, shift = PLANTED["T"], PLANTED["cycle"], planted_shift(w)
    found = {leg: [t for t in range(offset + shift, T, n) if t >= 1] for leg, offset in enumerate(planted_offsets())}
    assert all(w < t < T - 1 - w for frames in found.values() for t in frames)
    return found


def check_planted(r):
    """The planted walker's properties on one analysis r (the oracle's dict, or a device's result turned into one)."""
    P = PLANTED
    T, n = P["T"], P["cycle"]
    lift, _ = events(r["states"])
    planted = planted_lift_offs()
    assert planted_shift() == 0   # w = 2: the window moves no lift-off (x(c + 2) - x(c - 2) first exceeds 5 * 4 / fps at c = 0)
    for leg in range(6):
        assert np.flatnonzero(lift[:, leg]).tolist() == planted[leg], leg   # every planted lift-off to the frame, and no other
    # the steps: every pair of consecutive lift-offs but the one that spans the missing frames
    want = [(leg, t0, t2) for leg in range(6) for t0, t2 in zip(planted[leg][:-1], planted[leg][1:])
            if not (leg == P["missing_leg"] and t0 <= P["missing_frames"][0] < t2)]
    assert len(want) == sum(len(v) - 1 for v in planted.values()) - 1
    assert [(leg, t0, t2) for leg, t0, _, t2 in r["steps"].tolist()] == want
    assert np.all(r["steps"][:, 3] - r["steps"][:, 1] == n)
    mean, count = r["coupling"], r["coupling_count"]
    relative = np.arctan2(mean[..., 1], mean[..., 0]) / (2 * np.pi)
    offsets = planted_offsets()
    for i in range(6):
        for j in range(6):
            target = 0.0 if offsets[i] == offsets[j] else 0.5
            assert abs((relative[i, j] - target + 0.5) % 1.0 - 0.5) <= 0.02, (i, j, relative[i, j])
    classified = r["pattern_histogram"].sum()
    assert classified == (r["pattern"] >= 0).sum() >= T - 10
    assert r["pattern_histogram"][list(TRIPODS)].sum() >= 0.7 * classified


def planted_pose(golden_dir):
    """The golden recording's median pose [38, 3]; it holds every joint the walker needs."""
    pose = np.median(np.load(os.path.join(golden_dir, "golden_3d.npz"))["points3d_wo_procrustes"], axis=0)
    assert not missing(pose[TIPS]).any() and not missing(pose[COXAE]).any() and np.isfinite(jo.body_frame(pose)).all()
    return pose
