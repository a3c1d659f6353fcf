"""Device time of the trajectory triangulation (df3d_triangulate_trajectory) against df3d_triangulate on the same
input: 1 000 frames x 38 joints at the fly layout (7 cameras, the visibility of config.camera_see_joint, cell-quantised detections of
planted sinusoids, an outlier in one view of every 19th point).  Both entries are timed with device events round the C entry alone
(outputs and workspace allocated once, outside the window), after warm-ups, in --repeats windows of --window seconds each, the two
entries alternating; the median, the smallest and the largest window are reported, with the accepted iterations the fit's time includes.
The share of one banded solve spent in its serial part (the separators' system) comes from the device clock df3d_trajectory_solve
records at its phase boundaries, per block size.  --resources compiles the file once more with the compiler's resource report;
--resources-only needs no device.  The numbers gate nothing.

    python tests/perf/bench_trajectory.py [--frames 1000] [--blocks 0 64 ...] [--repeats 5] [--window 1.0] [--resources] [--out result.json]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

J = 38
BLOCKS = (3, 8, 16, 32, 64, 1 << 20)


def windows(calls, repeats, window_s, warmup=3):
    """ms per call of each of `calls`, [repeats] each, the entries alternating."""
    import torch

    out = [[] for _ in calls]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = []
    for fn in calls:
        for _ in range(warmup):
            fn()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        reps.append(int(min(20000, max(3, window_s * 1e3 / max(start.elapsed_time(stop), 1e-3)))))
    for _ in range(repeats):
        for k, fn in enumerate(calls):
            start.record()
            for _ in range(reps[k]):
                fn()
            stop.record()
            torch.cuda.synchronize()
            out[k].append(start.elapsed_time(stop) / reps[k])
    return out, reps


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def run(T, repeats, window_s, dev, blocks):
    import torch

    import trajectory_cases as tc
    from deepfly3d_amd import _native, config

    lib = _native.load()
    P, px, _ = tc.fly(T)
    ncam = px.shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    d = torch.from_numpy(px).to(dev)
    full = torch.empty((T, J, 3), dtype=torch.float64, device=dev)
    X = torch.empty_like(full)
    status = torch.empty((T, J), dtype=torch.int8, device=dev)
    weight = torch.empty((ncam, T, J), dtype=torch.float64, device=dev)
    err = torch.empty_like(weight)
    iterations = torch.empty((J,), dtype=torch.int32, device=dev)
    cost = torch.empty((J, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((J, 5), dtype=torch.int64, device=dev)
    lam = np.ascontiguousarray(config.TRAJECTORY_LAMBDA)
    dp = ctypes.POINTER(ctypes.c_double)

    def plain():
        _native.check(lib.df3d_triangulate(P.ctypes.data_as(ctypes.c_void_p), d.data_ptr(), ncam, T, J, full.data_ptr(), stream), "df3d_triangulate")

    def fit_with(block):
        need = lib.df3d_trajectory_work_bytes(ncam, T, J, block)
        work = torch.empty((need,), dtype=torch.uint8, device=dev)

        def fit():
            _native.check(lib.df3d_triangulate_trajectory(P.ctypes.data_as(dp), d.data_ptr(), full.data_ptr(), ncam, T, J, lam.ctypes.data_as(dp),
                                                          config.TRAJECTORY_HUBER, config.REPAIR_MAX_GAP, block, X.data_ptr(), status.data_ptr(),
                                                          weight.data_ptr(), err.data_ptr(), iterations.data_ptr(), cost.data_ptr(),
                                                          counts.data_ptr(), work.data_ptr(), need, stream), "df3d_triangulate_trajectory")

        return fit

    plain()
    out = {"frames": T, "joints": J, "ncam": ncam, "fits": [], "solves": []}
    for block in blocks:
        fit = fit_with(block)
        (t_plain, t_fit), reps = windows((plain, fit), repeats, window_s)
        torch.cuda.synchronize()
        it = iterations.cpu().numpy()
        out["fits"].append({"block_frames": block, "calls_per_window": reps, "windows": repeats, "df3d_triangulate": spread(t_plain),
                            "df3d_triangulate_trajectory": spread(t_fit), "ratio_of_medians": statistics.median(t_fit) / statistics.median(t_plain),
                            "accepted_iterations_max": int(it.max()), "accepted_iterations_mean": float(it.mean()),
                            "status_counts": counts.sum(dim=0).tolist()})
    # one banded solve at the fit's first iterate, its phases from the device clock it records (100 MHz)
    H = torch.empty((T, J, 6), dtype=torch.float64, device=dev)
    g = torch.empty((T, J, 3), dtype=torch.float64, device=dev)
    chain_cost = torch.empty((J,), dtype=torch.float64, device=dev)
    scratch = torch.empty((T * J,), dtype=torch.float64, device=dev)
    _native.check(lib.df3d_trajectory_linearize(P.ctypes.data_as(dp), d.data_ptr(), full.data_ptr(), ncam, T, J, config.TRAJECTORY_HUBER, H.data_ptr(),
                                                g.data_ptr(), weight.data_ptr(), err.data_ptr(), chain_cost.data_ptr(), scratch.data_ptr(), T * J * 8,
                                                stream), "df3d_trajectory_linearize")
    segment = torch.ones((T, J), dtype=torch.int8, device=dev)
    step = torch.empty((T, J, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((J,), dtype=torch.int32, device=dev)
    for block in blocks:
        need = lib.df3d_trajectory_work_bytes(1, T, J, block)
        work = torch.empty((need,), dtype=torch.uint8, device=dev)
        clock = torch.zeros((J, 4), dtype=torch.int64, device=dev)

        def solve():
            _native.check(lib.df3d_trajectory_solve(H.data_ptr(), g.data_ptr(), segment.data_ptr(), T, J, lam.ctypes.data_as(dp),
                                                    config.TRAJECTORY_MU_INIT, block, step.data_ptr(), ok.data_ptr(), clock.data_ptr(), work.data_ptr(), need,
                                                    stream),
                          "df3d_trajectory_solve")

        (t_solve,), reps = windows((solve,), repeats, window_s / 4)
        torch.cuda.synchronize()
        ticks = clock.cpu().numpy().astype(np.float64)
        phases = np.diff(ticks, axis=1)                      # interiors, separators, substitution, per chain
        share = phases[:, 1] / phases.sum(axis=1)
        out["solves"].append({"block_frames": block, "df3d_trajectory_solve": spread(t_solve), "calls_per_window": reps,
                              "separator_share_median": float(np.median(share)), "separator_share_max": float(share.max()),
                              "phase_ticks_median": [float(v) for v in np.median(phases, axis=0)]})
    return out


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd, sgpr_spills, vgpr_spills} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "trajectory.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", os.path.join(tmp, "x.o"),
               "-Rpass-analysis=kernel-resource-usage"]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=tmp).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes", "ScratchSize [bytes/lane]": "scratch_bytes",
            "Occupancy [waves/SIMD]": "waves_per_simd", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills"}
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"\d+(linearize_kernel|chain_sum_kernel|solve_kernel|fit_kernel)", m.group(1))
            name = k.group(1) if k else None
            if name:
                out[name] = {}
            continue
        m = re.search(r"(?:remark:|:\d+:\d+:)\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
        if m and name and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, nargs="*", default=None, help="block sizes; 0 is config.trajectory_block_frames(frames)")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        from deepfly3d_amd import config

        blocks = [b or config.trajectory_block_frames(a.frames) for b in (BLOCKS if a.blocks is None else a.blocks)]
        res["run"] = run(a.frames, a.repeats, a.window, dev, blocks)
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
