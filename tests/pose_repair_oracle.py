"""Float64 statement of the pose repair in plain numpy: a Hampel test of every joint against the median of its
own window, one pass, then linear filling of the short gaps that missing joints and outliers leave.  The model is this project's own
specification; it claims no parity with anything.  The medians are written out (a sort with the invalid samples at the end, then the
middle entries); numpy.median is never called.  Every number is formed by the operations the model names, one at a time, so that a
device built without multiply-add fusion gives the same bits.

Two forms of every stage: a vectorised one over sliding windows, which the device is compared with at every size, and a plain loop
over (frame, joint), which the vectorised one is compared with at small sizes.  Also here: the planted walker with noise and spikes."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import gait_oracle as go

HALF = 5            # config.REPAIR_HALF_WINDOW
K = 6.0             # config.REPAIR_THRESHOLD
FLOOR = 0.05        # config.REPAIR_FLOOR
N_MIN = 3           # config.REPAIR_MIN_COUNT
MAX_GAP = 10        # config.REPAIR_MAX_GAP
MAD_TO_SIGMA = 1.4826
TILE = 256          # csrc/pose_repair.hip: the frames of one block of the outlier test, and the lanes of one block of the scan
KEPT, MISSING_FILLED, OUTLIER_FILLED, MISSING_LEFT, OUTLIER_REMOVED = range(5)
CHUNK = 4096        # frames per slab of the vectorised test: bounds the memory of the windows

missing = go.missing


def median_sorted(v):
    """The model's median of the values v, sorted ascending: v[(n - 1) / 2] for an odd count, the mean of the two middle ones else."""
    n = len(v)
    return v[(n - 1) // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) * 0.5


def _window_median(values, valid, n):
    """values, valid [..., W] and n = valid.sum(-1): the median of the valid entries of every window.  The invalid ones are put at
    +inf (every valid one is finite) and so sorted to the end; a window without a valid entry gives a number nobody reads."""
    s = np.sort(np.where(valid, values, np.inf), axis=-1)
    k1, k2 = np.maximum((n - 1) // 2, 0), n // 2
    v1 = np.take_along_axis(s, k1[..., None], axis=-1)[..., 0]
    v2 = np.take_along_axis(s, np.minimum(k2, s.shape[-1] - 1)[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(n % 2 == 1, v1, (v1 + v2) * 0.5)


def outliers(X, h=HALF, k=K, floor=FLOOR, n_min=N_MIN):
    """X [T, 38, 3] -> (flags [T, 38] uint8: bit 0 missing, bit 1 outlier; score [T, 38])."""
    X = np.asarray(X, dtype=np.float64)
    T, W = len(X), 2 * h + 1
    scale = k * MAD_TO_SIGMA   # formed once
    miss = missing(X)
    flags, score = miss.astype(np.uint8), np.full((T, 38), np.nan)
    valid = np.zeros((T + 2 * h, 38), dtype=bool)   # a frame outside the recording is not valid: the clipped window
    valid[h:h + T] = ~miss
    padded = np.zeros((T + 2 * h, 38, 3))
    padded[h:h + T] = np.where(miss[..., None], 0.0, X)   # an invalid sample is never read: its place holds a finite number
    for t0 in range(0, T, CHUNK):
        t1 = min(t0 + CHUNK, T)
        vw = sliding_window_view(valid[t0:t1 + 2 * h], W, axis=0)   # [frames, 38, W]
        n = vw.sum(axis=-1)
        flagged, best = np.zeros(n.shape, dtype=bool), None
        for c in range(3):
            xw = sliding_window_view(padded[t0:t1 + 2 * h, :, c], W, axis=0)
            m = _window_median(xw, vw, n)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                dev = np.abs(xw - m[..., None])   # one subtraction
                mad = _window_median(dev, vw, n)
                thr = np.maximum(scale * mad, floor)   # one product
                dev_t = dev[..., h]
                flagged |= dev_t > thr
                r = np.where(dev_t == 0.0, 0.0, np.where(thr == 0.0, np.inf, dev_t / thr))   # one division
            best = r if c == 0 else np.where(r > best, r, best)   # the largest in order of c, by plain >
        tested = ~miss[t0:t1] & (n >= n_min)
        flags[t0:t1] |= (tested & flagged).astype(np.uint8) << 1
        score[t0:t1] = np.where(tested, best, np.nan)
    return flags, score


def outliers_loop(X, h=HALF, k=K, floor=FLOOR, n_min=N_MIN):
    """The same, window by window in Python: what `outliers` is checked against at small sizes."""
    X = np.asarray(X, dtype=np.float64)
    T = len(X)
    scale = k * MAD_TO_SIGMA
    miss = missing(X)
    flags, score = miss.astype(np.uint8), np.full((T, 38), np.nan)
    for t in range(T):
        a, b = max(t - h, 0), min(t + h, T - 1)
        for j in range(38):
            if miss[t, j]:
                continue
            V = [s for s in range(a, b + 1) if not miss[s, j]]
            if len(V) < n_min:
                continue
            best, flagged = None, False
            for c in range(3):
                x = [float(X[s, j, c]) for s in V]
                m = median_sorted(sorted(x))
                dev = [abs(v - m) for v in x]
                mad = median_sorted(sorted(dev))
                thr = max(scale * mad, floor)
                dev_t = abs(float(X[t, j, c]) - m)
                flagged = flagged or dev_t > thr
                r = 0.0 if dev_t == 0.0 else (np.inf if thr == 0.0 else dev_t / thr)
                best = r if c == 0 or r > best else best
            flags[t, j] |= 2 if flagged else 0
            score[t, j] = best
    return flags, score


def fill_gaps(X, flags, max_gap=MAX_GAP):
    """X [T, 38, 3], flags [T, 38] -> (Y [T, 38, 3], status [T, 38] int8, counts [38, 5] int64).  A joint is bad where its flags are
    not 0 (bit 0 decides the code where both bits are set)."""
    X, flags = np.asarray(X, dtype=np.float64), np.asarray(flags)
    T = len(X)
    good = flags == 0
    t = np.arange(T)[:, None]
    last = np.maximum.accumulate(np.where(good, t, -1), axis=0) if T else np.zeros((0, 38), dtype=np.int64)
    first = np.minimum.accumulate(np.where(good, t, T)[::-1], axis=0)[::-1] if T else last
    filled = ~good & (last >= 0) & (first < T) & (first - last - 1 <= max_gap)
    Y = X.copy()
    Y[~good] = 0.0
    tt, jj = np.nonzero(filled)
    a, b = last[tt, jj], first[tt, jj]
    A, B = X[a, jj], X[b, jj]
    w = (tt - a).astype(np.float64) / (b - a).astype(np.float64)   # one division
    Y[tt, jj] = A + (B - A) * w[:, None]                           # one subtraction, one product, one sum
    was_missing = (flags & 1) != 0
    status = np.where(good, KEPT, np.where(was_missing, np.where(filled, MISSING_FILLED, MISSING_LEFT),
                                           np.where(filled, OUTLIER_FILLED, OUTLIER_REMOVED))).astype(np.int8)
    counts = np.stack([(status == code).sum(axis=0) for code in range(5)], axis=1).astype(np.int64).reshape(38, 5)
    return Y, status, counts


def fill_gaps_loop(X, flags, max_gap=MAX_GAP):
    """The same by a walk along every joint's series: what `fill_gaps` is checked against."""
    X, flags = np.asarray(X, dtype=np.float64), np.asarray(flags)
    T = len(X)
    Y, status = X.copy(), np.zeros((T, 38), dtype=np.int8)
    for j in range(38):
        for t in range(T):
            if flags[t, j] == 0:
                continue
            a = next((s for s in range(t - 1, -1, -1) if flags[s, j] == 0), None)
            b = next((s for s in range(t + 1, T) if flags[s, j] == 0), None)
            filled = a is not None and b is not None and b - a - 1 <= max_gap
            if filled:
                w = np.float64(t - a) / np.float64(b - a)
                Y[t, j] = X[a, j] + (X[b, j] - X[a, j]) * w
            else:
                Y[t, j] = 0.0
            status[t, j] = (MISSING_FILLED if filled else MISSING_LEFT) if flags[t, j] & 1 else (OUTLIER_FILLED if filled else OUTLIER_REMOVED)
    counts = np.stack([(status == code).sum(axis=0) for code in range(5)], axis=1).astype(np.int64).reshape(38, 5)
    return Y, status, counts


def repair(X, h=HALF, k=K, floor=FLOOR, max_gap=MAX_GAP, n_min=N_MIN):
    """The whole stage, a dict."""
    flags, score = outliers(X, h, k, floor, n_min)
    points, status, counts = fill_gaps(X, flags, max_gap)
    return dict(flags=flags, score=score, points=points, status=status, counts=counts)


# ---------------------------------------------------------------------------------------------------------------------- test inputs
def tied_poses(T, h, seed=0):
    """gait_oracle.random_poses with planted ties and gaps: joint 3 constant for a run longer than the window, joint 5 with half of
    every window identical (the value repeats every other frame), joint 7 in steps of 3 frames; joint 11 missing throughout; joint
    13 with gaps of many lengths, two of them across a tile edge and a scan-block edge; joint 17 good only in the last frame of
    every block of 256 and the first of the next; joint 19 with a signed zero among ordinary values; joint 21 constant but for lone
    frames one unit off, a window and a half apart."""
    rng = np.random.default_rng(seed)
    X = go.random_poses(T, seed=seed)
    if T > 2:
        run = min(T, 3 * (2 * h + 1))
        s = int(rng.integers(0, T - run + 1))
        X[s:s + run, 3] = X[s, 3]
        X[::2, 5] = X[0, 5]
        X[:, 7] = X[(np.arange(T) // 3) * 3, 7]
        X[:, 11] = 0.0
        for s in rng.integers(0, T, size=max(T // 40, 2)):
            X[s:s + int(rng.integers(1, 16)), 13] = 0.0
        for edge in range(TILE, T, TILE):
            X[edge - 3:edge + 4, 13] = np.nan   # across the edge of a tile, which is the edge of a scan block too
        X[:, 17] = 0.0
        for edge in range(TILE, T + 1, TILE):
            X[edge - 1, 17] = rng.normal(size=3)
            if edge < T:
                X[edge, 17] = rng.normal(size=3)
        X[rng.integers(0, T, size=max(T // 20, 1)), 19, 1] = -0.0
        X[:, 21] = X[0, 21]
        X[h + 1::3 * (2 * h + 1), 21, 0] += 1.0   # lone steps off a constant: mad = 0, so with floor = 0 a score of +inf
    return X


def noisy_walker(median_pose, sigma=0.005, seed=0):
    """gait_oracle.planted_walker with N(0, sigma) noise on every coordinate; its two zeroed frames stay missing."""
    X = go.planted_walker(median_pose)
    gone = missing(X)
    X = X + np.random.default_rng(seed).normal(0.0, sigma, X.shape)
    X[gone] = 0.0
    return X


def planted_spikes(X, h, count=60, seed=1):
    """(X with `count` spikes, their (frame, joint) pairs): each in one random coordinate of a joint that is not missing, +-8 mm on
    a leg tip and +-1 mm elsewhere, no two within 2 h frames of each other on one joint."""
    rng = np.random.default_rng(seed)
    X, T = X.copy(), len(X)
    gone, placed = missing(X), []
    while len(placed) < count:
        t, j, c = int(rng.integers(0, T)), int(rng.integers(0, 38)), int(rng.integers(0, 3))
        sign = 1.0 if rng.random() < 0.5 else -1.0
        if gone[t, j] or any(q == j and abs(s - t) <= 2 * h for s, q in placed):
            continue
        X[t, j, c] += sign * (8.0 if j in go.TIPS else 1.0)
        placed.append((t, j))
    return X, placed
