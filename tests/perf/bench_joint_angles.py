"""Device time of the joint-angle pass: df3d_joint_angles on the golden recording tiled to --frames poses, with
one frame for the recording and with one frame per pose, and df3d_body_frame, timed with device events (20 launches after 3
warm-ups), in us per launch and as a fraction of 8 TB/s under the byte model of section 14.

    python tests/perf/bench_joint_angles.py [--frames 1000 100000] [--out result.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import _native, ops  # noqa: E402

HBM = 8e12   # bytes per second
READ_LEGS, READ_FRAME, WRITE_ANGLES, WRITE_LENGTHS = 6 * 15 * 8, 9 * 8, 6 * 8 * 8, 6 * 4 * 8   # bytes per pose: 720 (+ 72) read, 576 written
READ_COXAE = 6 * 3 * 8


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
    one, each = ops.body_frame(X[:1]), ops.body_frame(X)
    angles = torch.empty((T, 6, 8), dtype=torch.float64, device=dev)
    lengths = torch.empty((T, 6, 4), dtype=torch.float64, device=dev)
    frames = torch.empty((T, 3, 3), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(F):
        return lambda: _native.check(lib.df3d_joint_angles(X.data_ptr(), T, F.data_ptr(), F.shape[0], angles.data_ptr(), lengths.data_ptr(), stream),
                                     "df3d_joint_angles")

    def body():
        _native.check(lib.df3d_body_frame(X.data_ptr(), T, frames.data_ptr(), stream), "df3d_body_frame")

    out = {}
    written = WRITE_ANGLES + WRITE_LENGTHS
    for name, fn, nbytes, grid in (("joint_angles_kernel", run(one), READ_LEGS + written, [(T + 63) // 64, 384]),
                                   ("joint_angles_kernel_per_frame", run(each), READ_LEGS + READ_FRAME + written, [(T + 63) // 64, 384]),
                                   ("body_frame_kernel", body, READ_COXAE + READ_FRAME, [(T + 255) // 256, 256])):
        us = timed(fn)
        out[name] = {"frames": T, "grid": grid, "bytes_per_frame": nbytes, "us": us, "us_per_1000_frames": us * 1000.0 / T,
                     "fraction_of_8TBps": nbytes * T / (us * 1e-6) / HBM}
    return out


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
