"""Device time of the constant-length leg fit: df3d_leg_fit on the golden recording tiled to --frames poses with
its median lengths, anchored per frame, timed with device events (20 launches after 3 warm-ups) at the default max_iter and at
max_iter = 0..5 -- the time against the number of passes every lane makes separates the bytes (max_iter = 0: read, replay, write) from
the arithmetic (the slope) and from the wait for a wave's slowest lane (the default against the max_iter that equals the largest
iteration count) -- with the iteration counts, the bytes per frame and the fp64 operation count of section 15.

    python tests/perf/bench_leg_fit.py [--frames 1000 100000] [--out result.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import _native, ops  # noqa: E402
from deepfly3d_amd.config import RIGID_LEGS_MAX_ITER  # noqa: E402

HBM = 8e12                                   # bytes per second
FP64_VECTOR = 78.6e12                        # flop per second, vector fp64 with every operation a multiply-add
BYTES_PER_FRAME = 720 + 720 + 48 + 48        # the legs read and written, cost, info
FLOP_PER_PASS = 1700                         # one pass of the loop for one leg: ~1 100 fp64 instructions, a multiply-add counted twice (section 15)


def golden(T):
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "golden_3d.npz"))
    return np.ascontiguousarray(np.tile(g3["points3d_wo_procrustes"], (T // 15 + 1, 1, 1))[:T])


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
    X = torch.from_numpy(golden(T)).to(dev)
    L = np.ascontiguousarray(ops.segment_length_medians(X[:15]).cpu().numpy())
    out = X.clone()
    cost = torch.empty((T, 6), dtype=torch.float64, device=dev)
    info = torch.empty((T, 6, 2), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    Lp = L.ctypes.data_as(ctypes.c_void_p)

    def run(max_iter):
        return lambda: _native.check(lib.df3d_leg_fit(X.data_ptr(), T, Lp, None, max_iter, out.data_ptr(), cost.data_ptr(), info.data_ptr(), stream),
                                     "df3d_leg_fit")

    res = {"frames": T, "grid": [(T + 63) // 64, 384], "bytes_per_frame": BYTES_PER_FRAME, "flop_per_pass": FLOP_PER_PASS, "max_iter": {}}
    for max_iter in (RIGID_LEGS_MAX_ITER, 0, 1, 2, 3, 4, 5):
        us = timed(run(max_iter))
        iters = info[..., 1].to(torch.float64)
        passes = float(iters.sum())   # on this recording no trial is rejected: a pass is an accepted iteration
        res["max_iter"][str(max_iter)] = {"us": us, "us_per_1000_frames": us * 1000.0 / T, "iterations_mean": float(iters.mean()),
                                          "iterations_max": int(iters.max()), "status": sorted(set(info[..., 0].flatten().tolist())),
                                          "fraction_of_8TBps": BYTES_PER_FRAME * T / (us * 1e-6) / HBM,
                                          "fraction_of_fp64_vector_peak": FLOP_PER_PASS * passes / (us * 1e-6) / FP64_VECTOR}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernels": [kernels(T, dev) for T in a.frames]}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
