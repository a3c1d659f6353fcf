"""Seeded inputs for the camera-lag stage (csrc/sync.hip): the cameras of deepfly3d_amd/data/calib.npz, 3-D random
walks of the joints each camera sees under the fly layout (csrc/geometry_dev.h: relayout_source), projected, with +-0.5 px of uniform
noise, and a camera's frames shifted by a planted lag.  Host numpy only.  TEST INFRASTRUCTURE ONLY."""
import functools
import os

import numpy as np

T, J, NCAM = 96, 38, 7
MAX_LAG, WINDOW = 4, 16           # six windows of 16 frames; the jump of PLANTS["jump"] falls on a window's first frame
STEP_MM = 0.02                     # a joint's step per frame and axis: about 2.7 px at the rig's 137 px / mm
SPREAD_MM = 1.0
FOCUS = np.array([0.367, 0.142, -0.503])   # the point nearest the seven optical axes
MARGIN = 8                         # frames of the walk before frame 0 and after frame T - 1: a shifted camera shows them
# name -> (camera, lag before JUMP_AT, lag from JUMP_AT on): camera c shows instant t in its frame t + lag
JUMP_AT = 48
PLANTS = {"late": (1, 2, 2), "jump": (5, 0, -1), "none": (0, 0, 0)}


def cameras():
    """P [7, 3, 4] float64 of the packaged calibration."""
    import deepfly3d_amd

    c = np.load(os.path.join(os.path.dirname(deepfly3d_amd.__file__), "data", "calib.npz"))
    return np.ascontiguousarray(np.stack([c["intr"][i] @ np.concatenate([c["R"][i], c["tvec"][i][:, None]], axis=1) for i in range(NCAM)]))


def visible():
    """[7, 38] bool: the fly layout with the cameras in order: 0 .. 2 see joints 0 .. 18 (camera 2 only below 15), 4 .. 6 see 19 .. 37
    (camera 4 only below 34), camera 3 sees none."""
    see = np.zeros((NCAM, J), dtype=bool)
    see[0:3, :19] = True
    see[4:7, 19:] = True
    see[2, 15:] = False
    see[4, 34:] = False
    return see


def project(P, X):
    """(row_px, col_px) [C, n, J, 2] of X [n, J, 3]."""
    h = np.einsum("cik,njk->cnji", P[:, :, :3], X) + P[:, None, None, :, 3]
    return np.stack([h[..., 1] / h[..., 2], h[..., 0] / h[..., 2]], axis=-1)


@functools.lru_cache(maxsize=None)
def walk(seed=0):
    """(clean [7, T + 2 MARGIN, 38, 2], X [T + 2 MARGIN, 38, 3]): every camera's noisy detections of every frame of the walk, zeros where
    the camera does not see the joint.  Frame MARGIN of the walk is instant 0.  Read only."""
    rng = np.random.default_rng(2800 + seed)
    n = T + 2 * MARGIN
    X = FOCUS + rng.uniform(-SPREAD_MM, SPREAD_MM, size=(1, J, 3)) + np.cumsum(rng.normal(0.0, STEP_MM, size=(n, J, 3)), axis=0)
    px = project(cameras(), X) + rng.uniform(-0.5, 0.5, size=(NCAM, n, J, 2))
    px[~np.broadcast_to(visible()[:, None, :], px.shape[:3])] = 0.0
    assert (px[np.broadcast_to(visible()[:, None, :], px.shape[:3])] > 1.0).all()
    px.setflags(write=False)
    X.setflags(write=False)
    return px, X


@functools.lru_cache(maxsize=None)
def planted(name, seed=0):
    """(px [7, T, 38, 2], clean [7, T, 38, 2], lag [7, nW] int32): the recording with PLANTS[name], the same without a lag, and the lag of
    every camera and window.  Read only."""
    cam, before, after = PLANTS[name]
    full = walk(seed)[0]
    clean = np.ascontiguousarray(full[:, MARGIN:MARGIN + T])
    px = clean.copy()
    lag = np.zeros((NCAM, T // WINDOW), dtype=np.int32)
    lag[cam] = np.where(np.arange(T // WINDOW) * WINDOW < JUMP_AT, before, after)
    # camera `cam` shows instant t in its frame t + lag(t): its frame s holds the instant s - lag.  Around the jump the lag of the
    # frame is that of the instant it shows: the frames up to JUMP_AT + before - 1 hold instants before JUMP_AT.
    s = np.arange(T)
    instant = np.where(s < JUMP_AT + before, s - before, s - after)
    px[cam] = full[cam, MARGIN + instant]
    for a in (px, clean, lag):
        a.setflags(write=False)
    return px, clean, lag


def status_of(name):
    """sync_status [7] of a plant: 0 for camera 3, 2 for the planted camera, 1 elsewhere."""
    cam, before, after = PLANTS[name]
    s = np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.int8)
    if before or after:
        s[cam] = 2
    return s
