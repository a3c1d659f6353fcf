"""Time of the bundle adjustment with and without a robust loss, on the 1 000-frame window of the benchmark
(deepfly3d_amd.synthetic.synthetic_ba_window: 106 k observations) and on the 15-frame golden sample, each with an outlier planted in
every 19th observation (40 px in a seeded direction):

  * whole solves: bundle_adjust(loss='linear') and bundle_adjust(loss='soft_l1', f_scale=config.BA_F_SCALE): wall milliseconds (the
    solve synchronises with the host once per outer iteration and once per trial, so wall time is what a caller waits for), evaluations,
    and the milliseconds PER EVALUATION of each;
  * one evaluation alone: df3d_ba_eval against df3d_ba_eval_robust (residuals + both Jacobian planes; the robust one also writes the
    weight plane) and df3d_vec_dot(f, f) against df3d_ba_robust_cost, with device events round the C entry, after warm-ups, in
    --repeats windows of --window seconds, the entries alternating; median, smallest and largest window.

The numbers gate nothing.

    python tests/perf/bench_ba_robust.py [--repeats 5] [--window 0.2] [--out profiles/ba_robust_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EVERY, SHIFT = 19, 40.0


def inputs(which):
    """(points2d_px [7, T, 38, 2] with the planted outliers, the number planted, R, tvec, intr of the shipped calibration)."""
    from deepfly3d_amd.config import load_calibration
    from deepfly3d_amd.synthetic import synthetic_ba_window

    g3 = np.load(os.path.join(ROOT, "tests", "golden", "golden_3d.npz"))
    cal = load_calibration()
    c = {k: np.stack([cal[i][k] for i in range(7)]) for k in ("R", "tvec", "intr")}
    if which == "window_1000":
        px = synthetic_ba_window(g3["points3d_wo_procrustes"], g3["R"], g3["tvec"], g3["intr"], 1000, 0, 0)
    else:
        px = g3["points2d"] * np.array([480.0, 960.0])
    px = np.ascontiguousarray(px, dtype=np.float64).copy()
    seen = (px[..., 0] != 0) & (px[..., 1] != 0)
    at = np.argwhere(seen.transpose(1, 2, 0) & (seen.sum(axis=0) >= 2)[..., None])[::EVERY]      # (frame, joint, camera) order
    angle = np.random.default_rng(19).uniform(0.0, 2.0 * np.pi, size=len(at))
    px[at[:, 2], at[:, 0], at[:, 1]] += SHIFT * np.stack([np.sin(angle), np.cos(angle)], axis=1)
    return px, len(at), c


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def solves(px, c, repeats, dev):
    import torch

    from deepfly3d_amd import config
    from deepfly3d_amd.bundle_adjust import bundle_adjust

    out = {}
    for name, kw in (("linear", {}), ("soft_l1", dict(loss="soft_l1", f_scale=config.BA_F_SCALE))):
        ms = []
        for rep in range(repeats + 2):       # two warm-ups (the first one pays the library load and the graph capture)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R, t, info = bundle_adjust(px, c["R"], c["tvec"], c["intr"], device=dev, return_info=True, **kw)
            torch.cuda.synchronize()
            if rep >= 2:
                ms.append(1e3 * (time.perf_counter() - t0))
        out[name] = dict(spread(ms), nfev=info["nfev"], njev=info["njev"], status=info["status"], lsmr_iters=info["lsmr_iters"], cost=info["cost"],
                         ms_per_evaluation=statistics.median(ms) / info["nfev"])
        if "weights" in info:
            w = info["weights"]
            out[name]["weights_below_half"] = int((w < 0.5).sum())
    out["ms_ratio"] = out["soft_l1"]["median_ms"] / out["linear"]["median_ms"]
    out["ms_per_evaluation_ratio"] = out["soft_l1"]["ms_per_evaluation"] / out["linear"]["ms_per_evaluation"]
    return out


def entries(px, c, repeats, window_s, dev):
    import torch

    from bench_consensus import windows
    from deepfly3d_amd import _native, config, ops
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, _Dev, _rotvec_from_matrix

    px_dev = torch.from_numpy(px).to(dev)
    prob = BAProblemDevice(px_dev, c["intr"], dev)
    dv = _Dev(prob)
    P = np.einsum("cij,cjk->cik", c["intr"], np.concatenate([c["R"], c["tvec"][..., None]], axis=-1))
    X0 = ops.triangulate(P, px_dev)
    cams = np.concatenate([np.stack([_rotvec_from_matrix(c["R"][k]) for k in range(7)]), c["tvec"]], axis=1).ravel()
    x = torch.cat([torch.from_numpy(cams).to(dev), X0.reshape(-1, 3)[prob.ok_dev].reshape(-1)])
    f, ft, w, Jc, Jp = dv.new(prob.m), dv.new(prob.m), dv.new(prob.m), dv.new(12 * prob.nobs), dv.new(6 * prob.nobs)
    code, C = _native.BA_LOSSES.index("soft_l1"), config.BA_F_SCALE
    dv.eval(x, ft, None, None)
    calls = (lambda: dv.eval(x, f, Jc, Jp), lambda: dv.eval_robust(x, code, C, f, Jc, Jp, w=w), lambda: dv.dot(ft, ft), lambda: dv.robust_cost(ft, code, C))
    (t_eval, t_robust, t_dot, t_cost), reps = windows(calls, repeats, window_s)
    traffic = (2 + 18) * 8 * prob.nobs             # bytes written by df3d_ba_eval: f and the two Jacobian planes
    return {"nobs": prob.nobs, "npts": prob.npts, "calls_per_window": reps, "df3d_ba_eval": spread(t_eval), "df3d_ba_eval_robust": spread(t_robust),
            "eval_ratio_of_medians": statistics.median(t_robust) / statistics.median(t_eval),
            "bytes_written": {"df3d_ba_eval": traffic, "df3d_ba_eval_robust": traffic + 16 * prob.nobs},
            "df3d_vec_dot": spread(t_dot), "df3d_ba_robust_cost": spread(t_cost),
            "cost_ratio_of_medians": statistics.median(t_cost) / statistics.median(t_dot)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "outlier_every": EVERY, "outlier_shift_px": SHIFT, "runs": {}}
    side = torch.cuda.Stream(device=dev)
    for which in ("window_1000", "sample_15"):
        px, planted, c = inputs(which)
        with torch.cuda.stream(side):
            res["runs"][which] = {"frames": px.shape[1], "planted": planted, "solve": solves(px, c, a.repeats, dev),
                                  "evaluation": entries(px, c, a.repeats, a.window, dev)}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
