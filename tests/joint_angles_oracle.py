"""Float64 restatement of the leg joint-angle model, in plain numpy loops: the body frame, the eight angles
and four segment lengths of every leg with their NaN rules, and a forward-kinematics constructor that builds a leg FROM its
angles, so that the oracle is not the only witness of the kernel.  The model is this project's own specification."""
import numpy as np

TINY = 1e-18                      # relative bound on a squared sine below which a direction is undefined
COXAE = [0, 5, 10, 19, 24, 29]    # body-coxa joints C[side][l] at index 3 side + l
NAMES = ["thc_yaw", "thc_pitch", "thc_roll", "ctr_pitch", "ctr_roll", "fti_pitch", "fti_roll", "tita_pitch"]
ROLLS, BENDS = [2, 4, 6], [3, 5, 7]


def leg_joints(leg):
    side, l = divmod(leg, 3)
    return [19 * side + 5 * l + k for k in range(5)]


def missing(p):
    """All three coordinates exactly 0, or any of them not finite."""
    p = np.asarray(p, dtype=np.float64)
    return bool(np.all(p == 0.0) or not np.all(np.isfinite(p)))


def body_frame(pose):
    """pose [38, 3] -> [3, 3], rows ex, ey, ez; all NaN for a missing body-coxa joint or a degenerate set."""
    C = np.asarray(pose, dtype=np.float64)[COXAE].reshape(2, 3, 3)
    bad = np.full((3, 3), np.nan)
    if any(missing(c) for c in C.reshape(6, 3)):
        return bad
    cmax = max(float(c @ c) for c in C.reshape(6, 3))
    d = C[0].sum(axis=0) / 3.0 - C[1].sum(axis=0) / 3.0   # side 1 to side 0
    if d @ d <= TINY * cmax:
        return bad
    ey = d / np.sqrt(d @ d)
    f = (C[0, 0] + C[1, 0]) / 2.0 - (C[0, 2] + C[1, 2]) / 2.0   # hind to front
    fp = f - (f @ ey) * ey
    if fp @ fp <= TINY * cmax:
        return bad
    ex = fp / np.sqrt(fp @ fp)
    return np.stack([ex, ey, np.cross(ex, ey)])


def body_frames(X):
    """X [T, 38, 3] -> [T, 3, 3]: every pose's own frame."""
    return np.stack([body_frame(x) for x in X]) if len(X) else np.zeros((0, 3, 3))


def recording_frame(X):
    """[3, 3]: the frame of the pose whose body-coxa coordinates are the temporal medians over all frames as they stand."""
    pose = np.zeros((38, 3))
    pose[COXAE] = np.median(np.asarray(X, dtype=np.float64)[:, COXAE], axis=0)
    return body_frame(pose)


def bend(u, v):
    n = np.cross(u, v)
    return float(np.arctan2(np.sqrt(n @ n), u @ v))


def tors(u, w, v):
    wu, wv = np.cross(w, u), np.cross(w, v)
    ww = w @ w
    if wu @ wu <= TINY * ww * (u @ u) or wv @ wv <= TINY * ww * (v @ v):
        return np.nan
    return float(np.arctan2(np.sqrt(ww) * (w @ np.cross(u, v)), wu @ wv))


def leg_vectors(P, F, side):
    """(q [4, 3] segment vectors in leg coordinates, present [4]: both end joints there) of the leg's joints P [5, 3]."""
    sigma = -1.0 if side else 1.0
    v = P[1:] - P[:-1]
    q = np.stack([v @ F[0], sigma * (v @ F[1]), v @ F[2]], axis=1)
    miss = [missing(p) for p in P]
    return q, v, np.array([not miss[k] and not miss[k + 1] for k in range(4)])


def leg_angles(P, F, side):
    """(angles [8], lengths [4]) of one leg: joints P [5, 3], frame F [3, 3]."""
    with np.errstate(invalid="ignore", over="ignore"):
        q, v, present = leg_vectors(np.asarray(P, dtype=np.float64), F, side)
        lengths = np.array([np.sqrt(v[k] @ v[k]) if present[k] else np.nan for k in range(4)])
        frame_ok = bool(np.all(np.isfinite(F)))
        ok = [bool(present[k]) and (v[k] @ v[k]) > 0.0 and frame_ok for k in range(4)]
        a, b, c, d = q
        out = np.full(8, np.nan)
        if ok[0]:
            out[0] = np.arctan2(a[1], np.hypot(a[0], a[2]))
            if a[0] * a[0] + a[2] * a[2] > TINY * (a @ a):
                out[1] = np.arctan2(a[0], -a[2])
        if ok[0] and ok[1]:
            out[2] = tors(np.array([0.0, 1.0, 0.0]), a, b)
            out[3] = bend(a, b)
        if ok[0] and ok[1] and ok[2]:
            out[4] = tors(a, b, c)
        if ok[1] and ok[2]:
            out[5] = bend(b, c)
        if ok[1] and ok[2] and ok[3]:
            out[6] = tors(b, c, d)
        if ok[2] and ok[3]:
            out[7] = bend(c, d)
    return out, lengths


def frames_for(X, body_frame="recording"):
    """[T, 3, 3]: the frames `body_frame` ("recording", "per_frame", [3, 3] or [T, 3, 3]) means for X."""
    T = len(X)
    if isinstance(body_frame, str):
        if body_frame == "per_frame":
            return body_frames(X)
        assert body_frame == "recording"
        return np.broadcast_to(recording_frame(X), (T, 3, 3)) if T else np.zeros((0, 3, 3))
    F = np.asarray(body_frame, dtype=np.float64)
    return np.broadcast_to(F, (T, 3, 3)) if F.ndim == 2 else F


def joint_angles(X, body_frame="recording"):
    """X [T, 38, 3] -> (angles [T, 6, 8], lengths [T, 6, 4])."""
    X = np.asarray(X, dtype=np.float64)
    F = frames_for(X, body_frame)
    angles, lengths = np.zeros((len(X), 6, 8)), np.zeros((len(X), 6, 4))
    for t in range(len(X)):
        for leg in range(6):
            angles[t, leg], lengths[t, leg] = leg_angles(X[t, leg_joints(leg)], F[t], leg // 3)
    return angles, lengths


def min_sine(X, body_frame="recording"):
    """The smallest sine that enters a tors() or thc_pitch's atan2 anywhere in X: how far the input is from a degenerate case."""
    X = np.asarray(X, dtype=np.float64)
    F = frames_for(X, body_frame)
    best = np.inf

    def sine(u, w):
        n = np.cross(w, u)
        return np.sqrt((n @ n) / ((w @ w) * (u @ u)))

    for t in range(len(X)):
        for leg in range(6):
            q, _, _ = leg_vectors(X[t, leg_joints(leg)], F[t], leg // 3)
            a, b, c, d = q
            best = min(best, sine(np.array([0.0, 1.0, 0.0]), a), sine(b, a), sine(a, b), sine(c, b), sine(b, c), sine(d, c))
    return float(best)


def wrap(x):
    """Angle differences wrapped to (-pi, pi]."""
    return -((-np.asarray(x) + np.pi) % (2.0 * np.pi) - np.pi)


# ------------------------------------------------------------------------------------------------------------------ forward kinematics
def _unit(v):
    return v / np.sqrt(v @ v)


def _next_direction(w, u, beta, rho):
    """cos(beta) w + sin(beta) (cos(rho) u_perp + sin(rho) w x u_perp): w the previous segment's unit vector, u_perp the unit
    projection of the reference u perpendicular to w."""
    up = _unit(u - (u @ w) * w)
    return np.cos(beta) * w + np.sin(beta) * (np.cos(rho) * up + np.sin(rho) * np.cross(w, up))


def leg_from_angles(angles8, lengths4, F, P0, side):
    """[5, 3]: the joints of the leg that starts at P0 and has these angles and lengths in frame F (rows ex, ey, ez, orthonormal)
    on side `side` -- the definitions of section 14 read in the other direction."""
    yaw, pitch, r1, b1, r2, b2, r3, b3 = [float(x) for x in angles8]
    a = np.array([np.cos(yaw) * np.sin(pitch), np.sin(yaw), -np.cos(yaw) * np.cos(pitch)])
    b = _next_direction(a, np.array([0.0, 1.0, 0.0]), b1, r1)
    c = _next_direction(b, a, b2, r2)
    d = _next_direction(c, b, b3, r3)
    F = np.asarray(F, dtype=np.float64)
    sigma = -1.0 if side else 1.0
    P = [np.asarray(P0, dtype=np.float64)]
    for q, length in zip((a, b, c, d), lengths4):
        P.append(P[-1] + float(length) * (q[0] * F[0] + sigma * q[1] * F[1] + q[2] * F[2]))
    return np.stack(P)


def canonical_coxae(rng=None):
    """[2, 3, 3] body-coxa joints C[side][l] whose frame is the identity: mirror images in y, front and hind at one height."""
    x, w, z = np.array([0.6, 0.0, -0.7]), np.array([0.35, 0.45, 0.4]), np.array([0.1, 0.0, 0.1])
    if rng is not None:
        x, w = x + rng.uniform(-0.05, 0.05, 3), w + rng.uniform(-0.05, 0.05, 3)
        z = z + np.array([0.0, rng.uniform(-0.05, 0.05), 0.0])
    return np.stack([np.stack([x, s * w, z], axis=1) for s in (1.0, -1.0)])


def random_fly(rng, T):
    """(X [T, 38, 3], angles [T, 6, 8], lengths [T, 6, 4]): flies built by forward kinematics in the identity frame from angles well
    away from every degenerate case (yaw in +-1.3, pitch in +-3, rolls in +-3.1, bends in [0.2, 2.9], lengths in [0.3, 1]); the
    antenna and stripe joints are filled with noise."""
    angles = np.zeros((T, 6, 8))
    angles[..., 0] = rng.uniform(-1.3, 1.3, (T, 6))
    angles[..., 1] = rng.uniform(-3.0, 3.0, (T, 6))
    angles[..., ROLLS] = rng.uniform(-3.1, 3.1, (T, 6, 3))
    angles[..., BENDS] = rng.uniform(0.2, 2.9, (T, 6, 3))
    lengths = rng.uniform(0.3, 1.0, (T, 6, 4))
    X = rng.normal(0.0, 1.0, (T, 38, 3))
    for t in range(T):
        C = canonical_coxae(rng)
        for leg in range(6):
            X[t, leg_joints(leg)] = leg_from_angles(angles[t, leg], lengths[t, leg], np.eye(3), C[leg // 3, leg % 3], leg // 3)
    return X, angles, lengths


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, [1, 0, 2]]
