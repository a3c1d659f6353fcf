"""Inputs of the tracking tests (tests/test_track_host.py, tests/test_gpu_track.py), seeded: tie-heavy random peaks and the planted
distractor.  Everything is laid out as ops.heatmap_peaks leaves it: count [C, T, J] int32, pts [C, T, J, K, 2] float32, val [C, T, J, K]
float32."""
import numpy as np

IMAGE_HW = (480, 960)   # pixels; a heat-map cell is 7.5 px on either axis


def tie_heavy(seed, C, T, J, K, dirty=True):
    """Coordinates on a 6 x 6 grid of heat-map cells (0 to 53 px apart: both sides of tau = 30), values in quarters, counts from 0 to K
    and sometimes beyond; `dirty`: some slots hold a NaN or an infinity in the value or in a coordinate.  Equal costs are the rule."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, K + 2, size=(C, T, J)).astype(np.int32)
    count[rng.random((C, T, J)) < 0.1] = 0
    cell = rng.integers(0, 6, size=(C, T, J, K, 2))
    pts = (cell / np.array([64.0, 128.0])).astype(np.float32)
    val = (rng.integers(0, 5, size=(C, T, J, K)) / 4.0).astype(np.float32)
    if dirty:
        bad = rng.random((C, T, J, K))
        val[bad < 0.03] = np.nan
        val[(bad >= 0.03) & (bad < 0.05)] = np.inf
        pts[..., 0][(bad >= 0.05) & (bad < 0.07)] = np.nan
        pts[..., 1][(bad >= 0.07) & (bad < 0.09)] = -np.inf
    return count, pts, val


def planted(seed=7, T=200, K=4, C=1, J=1, outshone=0.3):
    """(count, pts, val, truth [C, T, J]): the true peak drifts about 2 px per frame along the columns with a pixel of jitter; a stationary
    distractor 150 px away outshines it in `outshone` of the frames; two weak peaks lie anywhere.  Slots are sorted by falling value, as
    df3d_heatmap_peaks sorts them, so slot 0 is the arg-max; truth is the true peak's slot."""
    rng = np.random.default_rng(seed)
    H, W = IMAGE_HW
    count = np.full((C, T, J), K, np.int32)
    pts, val = np.zeros((C, T, J, K, 2), np.float32), np.zeros((C, T, J, K), np.float32)
    truth = np.zeros((C, T, J), np.int32)
    for c in range(C):
        for j in range(J):
            row0, col0 = rng.uniform(100, 300), rng.uniform(100, 300)
            for t in range(T):
                true_px = (row0 + rng.normal(0, 1.0), col0 + 2.0 * t + rng.normal(0, 1.0))
                loud = rng.random() < outshone
                px = [true_px, (row0 + 150.0, col0 + 200.0)] + [(rng.uniform(0, H), rng.uniform(0, W)) for _ in range(K - 2)]
                v = [rng.uniform(0.6, 0.8), rng.uniform(0.85, 0.95) if loud else rng.uniform(0.2, 0.5)] + list(rng.uniform(0.02, 0.15, K - 2))
                order = np.argsort(-np.array(v), kind="stable")
                pts[c, t, j] = (np.array(px)[order] / np.array([H, W])).astype(np.float32)
                val[c, t, j] = np.array(v, np.float32)[order]
                truth[c, t, j] = int(np.nonzero(order == 0)[0][0])
    return count, pts, val, truth


# ------------------------------------------------------------------------------------------------------------------ the sweep's families
# DESIGN.md section 22, "swept": tests/test_track_cases_host.py certifies on the oracle every condition that tests/test_gpu_track_sweep.py
# relies on; the device test only compares.
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SUBNORMAL = np.float32(1e-40)
T_DESIGNED = 70
SWEEP_BLOCKS = (1, 5, 16, 17, 32, 33, 64)                 # placeholders and designed ties
MANY_CHAINS = ((15, 1), (1, 16), (17, 1), (5, 51), (16, 16), (257, 1), (27, 19))   # (C, J): 15, 16, 17, 255, 256, 257 and 513 chains
MANY_T, MANY_BLOCKS, MANY_K = (1, 37), (5, 256), 4
HALFWAY_HW, HALFWAY_PARAMS = (512, 512), (32.0, 2.0 ** -11, 2.0 ** -19)   # (tau, w_motion, w_value)
HALFWAY_K, HALFWAY_T = (3, 16), 70
WEIGHTS = ((30.0, 1024.0, 1024.0), (30.0, 1024.0, 0.0), (1e-3, 1.0, 1.0), (1e6, 1.0, 1.0), (30.0, 2.0 ** -21, 2.0 ** -21),
           (30.0, 3 * 2.0 ** -21, 1.0))
WEIGHTS_T, WEIGHTS_K = (8, 70), 8
ODD_BLOCKS, ODD_K = (15, 17, 31, 33, 47, 255, 257, 513), (3, 16)
WIDE_GRID = dict(C=27, J=19, K=2, T=130, block_frames=1)   # 513 x 130 = 66 690 workgroups of the block and trace kernels
WIDE_GRID_WORK_BYTES = 147_320_448


def scattered(seed, C, T, J, K, image_hw=IMAGE_HW, clean=False):
    """General position.  Per chain a true peak walks about 5 px per frame and axis inside the image; every frame puts it (a pixel of
    jitter) into a slot of its own choosing and the other slots within +-48 px of it on either axis, so the jumps between two frames fall
    on both sides of tau = 30 (+-60 px was tried first and leaves fewer than a fifth of the jumps below tau).  One slot of a frame holds
    the top value, uniform on [1.5, 2.5]; the others lie below it by a gap that is uniform on (0, 1) for seven tenths of them and on
    (1, 2.5) for the rest, so values span about [-1, 2.5] and v_best - v falls on both sides of 1 whatever K is (values drawn uniformly
    cannot give K = 2 both a third of its valid slots below 1 and a tenth above: half of them are their frame's best).  Unless `clean`:
    a fifth of the counts are drawn from [-3, K + 3] (the others from [K - 1, K + 1], at least 2 where K allows), INT_MIN and INT_MAX are planted;
    3 % of the slots lie outside the image (a coordinate outside [0, 1]) and 1 % have a coordinate of magnitude 1e30 to 3e38, all
    finite and so valid; slots are dirty as in tie_heavy (NaN and infinities in values and coordinates), and a float32 subnormal and a
    -inf are planted among the values."""
    rng = np.random.default_rng(seed)
    H, W = image_hw
    count = np.full((C, T, J), K, np.int32)
    if not clean:
        count = np.maximum(rng.integers(K - 1, K + 2, size=(C, T, J)), min(K, 2)).astype(np.int32)
        wild = rng.random((C, T, J)) < 0.2
        count[wild] = rng.integers(-3, K + 4, size=int(wild.sum()))
    start = np.stack([rng.uniform(0.25 * H, 0.75 * H, (C, 1, J)), rng.uniform(0.25 * W, 0.75 * W, (C, 1, J))], axis=-1)
    truth = start + np.cumsum(rng.normal(0.0, 5.0, (C, T, J, 2)), axis=1)                      # [C, T, J, 2] pixels
    px = truth[:, :, :, None, :] + rng.uniform(-48.0, 48.0, (C, T, J, K, 2))
    own = rng.integers(0, K, size=(C, T, J))
    at_truth = np.arange(K) == own[..., None]
    px = np.where(at_truth[..., None], truth[:, :, :, None, :] + rng.normal(0.0, 1.0, (C, T, J, 1, 2)), px)
    top = rng.integers(0, K, size=(C, T, J))
    gap = np.where(rng.random((C, T, J, K)) < 0.7, rng.uniform(0.0, 1.0, (C, T, J, K)), rng.uniform(1.0, 2.5, (C, T, J, K)))
    gap[np.arange(K) == top[..., None]] = 0.0
    val = (rng.uniform(1.5, 2.5, (C, T, J, 1)) - gap).astype(np.float32)
    pts = (px / np.array([H, W], np.float64)).astype(np.float32)
    if not clean:
        far = rng.random((C, T, J, K))
        outside = far < 0.03
        pts[outside] += (rng.choice([-1.0, 1.0], size=(int(outside.sum()), 2)) * rng.uniform(1.0, 2.0, (int(outside.sum()), 2))).astype(np.float32)
        huge = (far >= 0.03) & (far < 0.04)
        pts[..., 0][huge] = (rng.choice([-1.0, 1.0], size=int(huge.sum())) * 10.0 ** rng.uniform(30.0, 38.5, int(huge.sum()))).astype(np.float32)
        bad = rng.random((C, T, J, K))
        val[bad < 0.03] = np.nan
        val[(bad >= 0.03) & (bad < 0.05)] = np.inf
        pts[..., 0][(bad >= 0.05) & (bad < 0.07)] = np.nan
        pts[..., 1][(bad >= 0.07) & (bad < 0.09)] = -np.inf
        if count.size >= 4:
            a, b = rng.choice(count.size, 2, replace=False)
            count.reshape(-1)[a], count.reshape(-1)[b] = INT_MIN, INT_MAX
        if val.size >= 8:
            a, b = rng.choice(val.size, 2, replace=False)
            val.reshape(-1)[a], val.reshape(-1)[b] = SUBNORMAL, -np.inf
    return count, pts, val


def halfway(seed, K, C=2, T=HALFWAY_T, J=3):
    """For HALFWAY_HW and HALFWAY_PARAMS: whole pixels (multiples of 1 / 512, exact in float32) within 12 px of a centre that walks up to
    2 px per frame, and values in quarters, one slot at the top and the others 1/4 to 3/2 below it.  Every product is exact: a pair cost
    times 2^20 is d^2 / 2 with d^2 an integer (most below tau^2 = 1024, half of them odd) and a unary cost times 2^20 is 2 min(gap, 1),
    so x.5 is common before rint and has to go to the even neighbour."""
    rng = np.random.default_rng(seed)
    count = np.full((C, T, J), K, np.int32)
    few = rng.random((C, T, J)) < 0.1
    count[few] = rng.integers(0, K + 1, size=int(few.sum()))
    centre = 256 + np.cumsum(rng.integers(-2, 3, size=(C, T, J, 1, 2)), axis=1)
    px = centre + rng.integers(-12, 13, size=(C, T, J, K, 2))
    pts = (px / 512.0).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64) * 512.0, px)
    quarters = rng.choice([1, 1, 1, 2, 3, 3, 3, 4, 5, 6], size=(C, T, J, K))
    quarters[np.arange(K) == rng.integers(0, K, size=(C, T, J))[..., None]] = 0
    val = ((rng.integers(6, 11, size=(C, T, J, 1)) - quarters) / 4.0).astype(np.float32)
    return count, pts, val


PLACEHOLDER_PATTERNS = ("every frame", "frame 0", "frame T - 1", "both sides of every block edge", "a whole chunk", "a whole ring", "every other frame",
                        "a valid frame between two runs")


def placeholder_frames(B, T=T_DESIGNED):
    """[len(PLACEHOLDER_PATTERNS), T] bool: the frames each pattern makes placeholders, at block size B."""
    t = np.arange(T)
    edges = np.zeros(T, bool)
    for b in range(1, -(-T // B)):
        edges[b * B - 1] = edges[b * B] = True
    return np.stack([np.ones(T, bool), t == 0, t == T - 1, edges, (t >= 16) & (t < 32), (t >= 16) & (t < 48), t % 2 == 1,
                     ((t >= 20) & (t < 40)) & (t != 30)])


def placeholders(seed, B, K=4, T=T_DESIGNED):
    """One chain per pattern of PLACEHOLDER_PATTERNS along J, on a clean `scattered` (every other frame has K valid slots).  A
    placeholder frame is made in one of three ways in turn: count 0, count INT_MIN, or a full count with every value NaN."""
    frames = placeholder_frames(B, T)
    count, pts, val = scattered(seed, 1, T, len(frames), K, clean=True)
    for j, row in enumerate(frames):
        for n, t in enumerate(np.nonzero(row)[0]):
            if n % 3 == 0:
                count[0, t, j] = 0
            elif n % 3 == 1:
                count[0, t, j] = INT_MIN
            else:
                val[0, t, j] = np.nan
    return count, pts, val


def tie_frames(B, T=T_DESIGNED):
    """The frames of `designed_ties` whose slot 0 is invalid: frame 3, block 0's last frame, block 1's first frame and the last frame."""
    return sorted({3, B - 1, min(B, T - 1), T - 1})


def designed_ties(B, T=T_DESIGNED):
    """test_reversed_lexicographic_ties_by_hand's construction across block edges: chain 0 has two slots and chain 1 three, all at one
    place with one value in every frame, so every path costs 0 and slot 0 wins throughout; in tie_frames(B) slot 0 is invalid (its value
    a NaN) and slot 1 wins there alone.  (count, pts, val, wanted choice [1, T, 2])."""
    count = np.zeros((1, T, 2), np.int32)
    count[..., 0], count[..., 1] = 2, 3
    pts = np.full((1, T, 2, 3, 2), 0.25, np.float32)
    val = np.full((1, T, 2, 3), 0.5, np.float32)
    wanted = np.zeros((1, T, 2), np.int32)
    for t in tie_frames(B, T):
        val[0, t, :, 0] = np.nan
        wanted[0, t] = 1
    return count, pts, val, wanted


# the seeds: chosen so that the oracle alone meets the conditions tests/test_track_cases_host.py asserts on every run
MANY_RETRIES = {(15, 1, 1): 4, (1, 16, 1): 3, (257, 1, 1): 1, (27, 19, 1): 3}   # one frame: the first seeds whose last chain leaves slot 0


def many_chains(C, J, T):
    return scattered(2000 + 100 * C + J + 7 * T + 1000 * MANY_RETRIES.get((C, J, T), 0), C, T, J, MANY_K)


def weights_case(T):
    return scattered(3000 + T, 2, T, 3, WEIGHTS_K)


def odd_block_times(B):
    return (B - 1, B, B + 1, 2 * B + 1)


def odd_blocks_case(K, T):
    return scattered(4000 + 10000 * K + T, 2, T, 3, K)


def wide_grid():
    w = WIDE_GRID
    return scattered(5000, w["C"], w["T"], w["J"], w["K"])


def scattered_instances():
    """{name: (count, pts, val)} of every `scattered` input the device tests use."""
    out = {f"many {C}x{J} T={T}": many_chains(C, J, T) for C, J in MANY_CHAINS for T in MANY_T}
    out.update({f"weights T={T}": weights_case(T) for T in WEIGHTS_T})
    out.update({f"odd K={K} T={T}": odd_blocks_case(K, T) for K in ODD_K for T in sorted({t for B in ODD_BLOCKS for t in odd_block_times(B)})})
    out["wide grid"] = wide_grid()
    return out
