"""Device time of the temporal smoothing pass: df3d_smooth_pose2d on the golden detections tiled to --frames
frames x 7 cameras, timed with device events (20 launches after 3 warm-ups), in us per launch and as a fraction of 8 TB/s on
bytes = 2 * C * T * 76 * 8 (one read and one write of the data); then the wall time of Core.smooth_points2d, host copies included.

    python tests/perf/bench_smooth.py [--frames 1000 100000] [--out result.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import _native, ops  # noqa: E402

HBM = 8e12   # bytes per second, the figure DESIGN.md section 10 uses
C, NCH, WINDOW = 7, 76, 20


def golden(T):
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "golden_3d.npz"))
    return np.ascontiguousarray(np.tile(g3["points2d"] * np.array([480.0, 960.0]), (1, T // 15 + 1, 1, 1))[:, :T]), g3


def timed(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps   # us per launch


def kernel(T, dev):
    lib = _native.load()
    px, _ = golden(T)
    pxd = torch.from_numpy(px).to(dev)
    out = torch.empty_like(pxd)
    ws, wk = ops.gaussian_window_taps(WINDOW, ops.SMOOTH_SIGMA), ops.gaussian_window_taps(WINDOW, ops.KEEP_SIGMA)
    dp = ctypes.POINTER(ctypes.c_double)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def smooth():
        _native.check(lib.df3d_smooth_pose2d(pxd.data_ptr(), C, T, NCH, WINDOW, 5.0, ws.ctypes.data_as(dp), wk.ctypes.data_as(dp), out.data_ptr(), stream),
                      "df3d_smooth_pose2d")

    us = timed(smooth)
    nbytes = 2 * C * T * NCH * 8
    kept = float((out == pxd).double().mean())
    return {"frames": T, "grid": [(T + 63) // 64, C, 256], "bytes": nbytes, "us": us, "us_per_1000_frames": us * 1000.0 / T,
            "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM, "share_of_outputs_kept": kept}


def core_wall(T, dev):
    from deepfly3d_amd.camera_network import CameraNetwork
    from deepfly3d_amd.core import Core

    px, g3 = golden(T)
    core = Core.__new__(Core)
    calib = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "intr": g3["intr"][c], "distort": g3["distort"][c]} for c in range(7)}
    core.camNet, core.device, core.is_primary, core.max_img_id = CameraNetwork(px, calib=calib, device=dev), dev, True, T - 1
    core.smooth_points2d(0)
    t0 = time.perf_counter()
    for _ in range(3):
        core.smooth_points2d(0, refresh=True)
    first = (time.perf_counter() - t0) * 1e3 / 3
    t0 = time.perf_counter()
    for c in range(7):
        core.smooth_points2d(c)
    return {"frames": T, "smooth_points2d_ms": first, "cached_seven_cameras_ms": (time.perf_counter() - t0) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernel": [kernel(T, dev) for T in a.frames], "core": [core_wall(T, dev) for T in a.frames]}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
