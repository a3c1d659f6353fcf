"""Device time of the plain and the sub-pixel arg-max on one device batch of the pipeline, 896 views x 19
planes of 64 x 128 float32 (558 MB: larger than the last-level cache, so every launch reads HBM): df3d_heatmap_argmax_checked beside
df3d_heatmap_argmax_subpixel, and df3d_heatmap_peaks beside df3d_heatmap_peaks_subpixel, on the same Gaussian-blob planes.  The two
kernels of a pair are timed in alternating windows of --launches launches with device events, after a warm-up of each; the median over
--rounds windows and their spread (min, max, and max - min over the median) are reported, the ratio refined / plain beside the spread
of the plain kernel.

    python tests/perf/bench_subpixel.py [--views 896] [--rounds 21] [--launches 100] [--out result.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import ops  # noqa: E402

HBM = 8e12   # bytes per second
J, H, W = 19, 64, 128


def blobs(views, dev, seed=0):
    """[views, 19, 64, 128] float32 Gaussian heat-maps (sigma 1.5 cells) with centres drawn uniformly inside the plane, made on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    cr = torch.rand((views, J, 1, 1), generator=g, device=dev, dtype=torch.float64) * (H - 7) + 3
    cc = torch.rand((views, J, 1, 1), generator=g, device=dev, dtype=torch.float64) * (W - 7) + 3
    r = torch.arange(H, device=dev, dtype=torch.float64).view(1, 1, H, 1)
    c = torch.arange(W, device=dev, dtype=torch.float64).view(1, 1, 1, W)
    out = torch.empty((views, J, H, W), dtype=torch.float32, device=dev)
    for lo in range(0, views, 64):   # in pieces: the float64 intermediate of the whole batch would be 1.1 GB
        out[lo : lo + 64] = torch.exp(-((r - cr[lo : lo + 64]) ** 2 + (c - cc[lo : lo + 64]) ** 2) / (2.0 * 1.5 * 1.5)).float()
    return out


def window(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches   # us per launch


def pair(plain, refined, rounds, launches, nbytes):
    for fn in (plain, refined):   # warm-up: code objects loaded, clocks up
        window(fn, launches)
    t = {"plain": [], "refined": []}
    for _ in range(rounds):       # alternating windows: both kernels see the same neighbours on the machine
        t["plain"].append(window(plain, launches))
        t["refined"].append(window(refined, launches))
    out = {}
    for name, v in t.items():
        v = np.asarray(v)
        med = float(np.median(v))
        out[name] = {"median_us": med, "min_us": float(v.min()), "max_us": float(v.max()), "spread": float((v.max() - v.min()) / med),
                     "fraction_of_8TBps": nbytes / (med * 1e-6) / HBM}
    out["ratio_refined_over_plain"] = out["refined"]["median_us"] / out["plain"]["median_us"]
    out["ratio_of_minima"] = out["refined"]["min_us"] / out["plain"]["min_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=896)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--peaks", type=int, default=10, help="k of the peaks pair; 0 skips it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    hm = blobs(a.views, dev)
    nbytes = hm.numel() * 4
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    p0, c0 = ops.heatmap_argmax(hm, nonfinite=flag)
    p1, c1 = ops.heatmap_argmax(hm, nonfinite=flag, subpixel=True)
    assert torch.equal(c0, c1) and float((p1 - p0).abs().max()) <= 0.5 / H and not torch.equal(p0, p1)
    res = {"device": torch.cuda.get_device_name(0), "planes": a.views * J, "plane": [H, W], "bytes_read": nbytes, "rounds": a.rounds,
           "launches_per_window": a.launches,
           "argmax": pair(lambda: ops.heatmap_argmax(hm, nonfinite=flag), lambda: ops.heatmap_argmax(hm, nonfinite=flag, subpixel=True),
                          a.rounds, a.launches, nbytes)}
    if a.peaks:
        res["peaks"] = {"k": a.peaks, **pair(lambda: ops.heatmap_peaks(hm, a.peaks), lambda: ops.heatmap_peaks(hm, a.peaks, subpixel=True),
                                             a.rounds, max(1, a.launches // 2), nbytes)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
