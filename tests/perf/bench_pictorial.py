"""Device time of the pictorial-structures correction: df3d_heatmap_peaks, df3d_ps_proposals and
df3d_ps_solve on seeded synthetic heat-maps (a Gaussian at every projected golden joint over uniform noise, so that every
plane has its K peaks: the largest proposal sets), timed with device events, in ms per 1 000 frames.

    python tests/perf/bench_pictorial.py [--frames 1000 12500] [--k 10] [--m 64] [--out result.json]

Heat-maps of 12 500 frames would need 53 GB: the peaks kernel runs over one resident block of `--block` frames as many
times as the frame count needs; proposals and solve run on the peaks of all frames (the block's tiled), in the chunks
ops.pictorial_correct uses."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import ops  # noqa: E402
from deepfly3d_amd.synthetic import synthetic_points2d  # noqa: E402
from oracle import geometry as og  # noqa: E402

ORDER = [0, 1, 2, 3, 4, 5, 6]


def heatmaps(block, dev, seed=0):
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "golden_3d.npz"))
    X = np.tile(g3["points3d_wo_procrustes"], (block // 15 + 1, 1, 1))[:block]
    p2 = synthetic_points2d(X, g3["R"], g3["tvec"], g3["intr"])               # [7, T, 38, 2] normalised, re-layout convention
    gen = torch.Generator(device=dev).manual_seed(seed)
    hm = torch.rand((7, block, 19, 64, 128), generator=gen, device=dev) * 0.3
    r = torch.arange(64, device=dev, dtype=torch.float32)[:, None]
    c = torch.arange(128, device=dev, dtype=torch.float32)[None, :]
    for cam in range(7):
        pos = ORDER.index(cam)
        if pos == 3:
            continue
        sl = slice(0, 19) if pos < 3 else slice(19, 38)
        rows = torch.from_numpy(p2[cam, :, sl, 0] * 64).to(dev, torch.float32)
        cols = torch.from_numpy(p2[cam, :, sl, 1] * 128).to(dev, torch.float32)
        if pos > 3:
            cols = 128 - cols
        g = torch.exp(-((r - rows[..., None, None]) ** 2 + (c - cols[..., None, None]) ** 2) / 4.5)
        hm[cam] += g
    return og.projection_matrices(g3["R"], g3["tvec"], g3["intr"]), hm.reshape(7 * block, 19, 64, 128).contiguous()


def timed(fn, reps=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1000, 12500])
    ap.add_argument("--block", type=int, default=250)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, hm = heatmaps(a.block, dev)
    count, pts, vals = ops.heatmap_peaks(hm, a.k)
    amp, _ = ops.heatmap_argmax(hm)
    results = []
    for T in a.frames:
        reps = (T + a.block - 1) // a.block

        def peaks():
            for _ in range(reps):
                ops.heatmap_peaks(hm, a.k)

        t_peaks = timed(peaks) * T / (reps * a.block)
        tile = lambda x: x.view(7, a.block, *x.shape[1:]).repeat(1, reps, *([1] * (x.dim() - 1)))[:, :T].contiguous()  # noqa: E731
        c, p, v = tile(count), tile(pts), tile(vals)
        am = ops.relayout_19_to_38(tile(amp), ORDER)
        chunk = 4096
        spans = [(t0, min(T, t0 + chunk)) for t0 in range(0, T, chunk)]
        kept = [ops.ps_proposals(P, ORDER, am, c, p, v, [960, 480], sp, a.m) for sp in spans]
        t_prop = timed(lambda: [ops.ps_proposals(P, ORDER, am, c, p, v, [960, 480], sp, a.m) for sp in spans])
        t_solve = timed(lambda: [ops.ps_solve(ORDER, am, c, p, kp, sp) for kp, sp in zip(kept, spans)])
        per_k = 1000.0 / T
        row = {"frames": T, "k": a.k, "m": a.m, "peaks_ms_per_1000": t_peaks * per_k, "proposals_ms_per_1000": t_prop * per_k,
               "solve_ms_per_1000": t_solve * per_k, "total_ms_per_1000": (t_peaks + t_prop + t_solve) * per_k,
               "mean_peaks_per_plane": float(count.float().mean())}
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
