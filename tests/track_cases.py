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
