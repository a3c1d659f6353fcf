"""Device time of the reprojection-error pass: df3d_reproj_errors beside df3d_triangulate on the same
frames (the golden recording tiled), timed with device events, in us per 1 000 frames and as a fraction of 8 TB/s; then the
wall time of Core.next_error on a recording of --scan frames, for an error in the next frame and for a scan that finds none.

    python tests/perf/bench_reproj.py [--frames 1000 100000] [--scan 100000] [--out result.json]
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
from oracle import geometry as og  # noqa: E402

HBM = 8e12   # bytes per second
READ_PX, READ_X, WRITE_ERR, WRITE_JMAX, WRITE_MASK = 7 * 38 * 16, 38 * 24, 7 * 38 * 8, 38 * 8, 8   # bytes per frame


def golden(T):
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "golden_3d.npz"))
    px = np.tile(g3["points2d"] * np.array([480.0, 960.0]), (1, T // 15 + 1, 1, 1))[:, :T]
    return og.projection_matrices(g3["R"], g3["tvec"], g3["intr"]), np.ascontiguousarray(px), g3


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


def kernels(T, dev):
    lib = _native.load()
    P, px, _ = golden(T)
    pxd = torch.from_numpy(px).to(dev)
    X = ops.triangulate(P, pxd)
    err = torch.empty((7, T, 38), dtype=torch.float64, device=dev)
    jmax = torch.empty((T, 38), dtype=torch.float64, device=dev)
    mask = torch.empty((T,), dtype=torch.int64, device=dev)
    thr = np.full(38, 40.0)
    dp = ctypes.POINTER(ctypes.c_double)
    Ph = np.ascontiguousarray(P)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def reproj():
        _native.check(lib.df3d_reproj_errors(Ph.ctypes.data_as(dp), pxd.data_ptr(), X.data_ptr(), 7, T, 38, thr.ctypes.data_as(dp), err.data_ptr(),
                                             jmax.data_ptr(), mask.data_ptr(), stream), "df3d_reproj_errors")

    def tri():
        _native.check(lib.df3d_triangulate(Ph.ctypes.data_as(ctypes.c_void_p), pxd.data_ptr(), 7, T, 38, X.data_ptr(), stream), "df3d_triangulate")

    out = {}
    for name, fn, nbytes in (("reproj_kernel", reproj, READ_PX + READ_X + WRITE_ERR + WRITE_JMAX + WRITE_MASK), ("triangulate_kernel", tri, READ_PX + READ_X)):
        us = timed(fn)
        out[name] = {"frames": T, "grid": [(T + 3) // 4 if name == "reproj_kernel" else (T * 38 + 255) // 256, 256], "bytes_per_frame": nbytes,
                     "us": us, "us_per_1000_frames": us * 1000.0 / T, "fraction_of_8TBps": nbytes * T / (us * 1e-6) / HBM}
    return out


def scan(T, dev):
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd.camera_network import CameraNetwork
    from deepfly3d_amd.core import Core

    _, px, g3 = golden(T)
    core = Core.__new__(Core)
    calib = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "intr": g3["intr"][c], "distort": g3["distort"][c]} for c in range(7)}
    core.camNet, core.device, core.is_primary, core.max_img_id = CameraNetwork(px, calib=calib, device=dev), dev, True, T - 1
    bad = core.next_error(0)   # the golden recording flags frame 2 (tiled every 15 frames): one chunk
    res = {"frames": T, "first_error_after_0": bad}
    t0 = time.perf_counter()
    for _ in range(10):
        core.next_error(0)
    res["next_error_near_ms"] = (time.perf_counter() - t0) * 100.0
    saved = cfg.REPROJ_THR.copy()
    cfg.REPROJ_THR[:] = np.inf   # nothing flagged: every chunk up to the end of the recording
    try:
        core.next_error(0)
        t0 = time.perf_counter()
        for _ in range(3):
            assert core.next_error(0) is None
        res["next_error_full_scan_ms"] = (time.perf_counter() - t0) * 1e3 / 3
    finally:
        cfg.REPROJ_THR[:] = saved
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--scan", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernels": [kernels(T, dev) for T in a.frames], "scan": scan(a.scan, dev) if a.scan else None}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
