"""Device time of the heat-map triangulation (df3d_triangulate_heatmaps): --frames frames x 38 joints at the fly
layout (the six cameras with planes, Gaussian blobs planted on the golden pose; --unique frames are planted and tiled on the device, a
frame's heat-maps being 3.7 MB).  Timed with device events round the C entry alone (outputs allocated once, outside the window), after
warm-ups, in --repeats windows of --window seconds each, the entries alternating: the search with its windows staged in LDS (the
default), the search reading the planes (budget 0), and df3d_triangulate on the projections of the same start points.  The stage's
real cost is the second pass of the network: --network times the f32 engine (synthetic weights) on one batch of 16 frames' six views
and scales it to --frames.  --resources compiles the file once more with the compiler's resource report; --resources-only needs no
device.  The numbers gate nothing.

    python tests/perf/bench_heatmap3d.py [--frames 1000] [--unique 25] [--repeats 5] [--window 1.0] [--network] [--resources] [--out result.json]
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

from bench_trajectory import spread, windows   # noqa: E402  (the same timing windows)

J = 38


def run(T, unique, repeats, window_s, dev, network):
    import torch

    import heatmap3d_cases as hc
    import heatmap3d_oracle as ho
    from deepfly3d_amd import _native, config

    lib = _native.load()
    frames = [hc.fly(15, seed=s) for s in range(-(-unique // 15))]
    tile = lambda key: np.concatenate([f[key] for f in frames])[:unique]   # noqa: E731
    case = frames[0]
    P, flip, plane = case["P"], np.ascontiguousarray(case["flip"]), np.ascontiguousarray(case["plane"])
    V, C, H, W = len(P), 19, hc.H, hc.W
    times = -(-T // unique)
    hm = torch.from_numpy(tile("hm")).to(dev).repeat(times, 1, 1, 1, 1)[:T].contiguous()
    X0_host = np.tile(tile("X0"), (times, 1, 1))[:T]
    X0 = torch.from_numpy(np.ascontiguousarray(X0_host)).to(dev)
    px = np.zeros((V, T, J, 2))
    for v in range(V):
        row, col, _ = ho.project(P[v], X0_host)
        px[v, ..., 0], px[v, ..., 1] = np.where(plane[v] >= 0, row, 0.0), np.where(plane[v] >= 0, col, 0.0)
    px = torch.from_numpy(px).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    levels = config.HEATMAP3D_LEVELS
    X = torch.empty((T, J, 3), dtype=torch.float64, device=dev)
    plain_X = torch.empty_like(X)
    score, shift = torch.empty((T, J), dtype=torch.float64, device=dev), torch.empty((T, J), dtype=torch.float64, device=dev)
    status, path = torch.empty((T, J), dtype=torch.int8, device=dev), torch.empty((T, J), dtype=torch.int8, device=dev)
    views = torch.empty((T, J), dtype=torch.int32, device=dev)
    choice = torch.empty((T, J, levels), dtype=torch.int32, device=dev)
    counts = torch.empty((J, 4), dtype=torch.int64, device=dev)
    dp, bp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
    cell = ho.cell_size(hc.IMAGE_SHAPE, H, W)
    budget = lib.df3d_heatmap3d_window_doubles()

    def search_with(cells):
        def search():
            _native.check(lib.df3d_triangulate_heatmaps(hm.data_ptr(), T, V, C, H, W, P.ctypes.data_as(dp), flip.ctypes.data_as(bp),
                                                        plane.ctypes.data_as(ip), J, X0.data_ptr(), config.HEATMAP3D_HALF, levels, cell[0], cell[1],
                                                        float(np.log(config.HEATMAP3D_FLOOR)), cells, X.data_ptr(), score.data_ptr(),
                                                        status.data_ptr(), views.data_ptr(), shift.data_ptr(), choice.data_ptr(), counts.data_ptr(),
                                                        path.data_ptr(), stream), "df3d_triangulate_heatmaps")

        return search

    def plain():
        _native.check(lib.df3d_triangulate(P.ctypes.data_as(ctypes.c_void_p), px.data_ptr(), V, T, J, plain_X.data_ptr(), stream), "df3d_triangulate")

    staged, planes = search_with(budget), search_with(0)
    (t_staged, t_planes, t_plain), reps = windows((staged, planes, plain), repeats, window_s)
    staged()
    torch.cuda.synchronize()
    out = {"frames": T, "joints": J, "views": V, "unique_frames": unique, "levels": levels, "half_mm": config.HEATMAP3D_HALF,
           "window_doubles": budget, "calls_per_window": reps, "windows": repeats, "df3d_triangulate_heatmaps": spread(t_staged),
           "df3d_triangulate_heatmaps_budget_0": spread(t_planes), "df3d_triangulate": spread(t_plain),
           "planes_over_lds": statistics.median(t_planes) / statistics.median(t_staged),
           "search_over_df3d_triangulate": statistics.median(t_staged) / statistics.median(t_plain),
           "status_counts": counts.sum(dim=0).tolist(), "staged_searches": int((path == 1).sum()), "plane_searches": int((path == 2).sum()),
           "largest_shift_mm": float(shift.max())}
    if network:
        os.environ.setdefault("DF3D_SYNTHETIC_WEIGHTS", "0")
        from deepfly3d_amd.inference import PREPROCESS, get_engine

        engine = get_engine(dtype="f32", device=dev)
        luma = torch.randint(0, 256, (16 * V, hc.IMAGE_SHAPE[1], hc.IMAGE_SHAPE[0]), dtype=torch.uint8, device=dev)
        f = torch.from_numpy(flip).to(dev).repeat(16)
        (t_net,), net_reps = windows((lambda: engine.forward_u8(luma, f, PREPROCESS["mean"], PREPROCESS["std"], resize=PREPROCESS["resize"]),),
                                     repeats, window_s)
        out["network_f32_16_frames"] = spread(t_net)
        out["network_f32_scaled_to_frames_ms"] = statistics.median(t_net) * T / 16.0
        out["network_over_search"] = out["network_f32_scaled_to_frames_ms"] / statistics.median(t_staged)
    return out


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd, sgpr_spills, vgpr_spills} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "heatmap3d.hip")
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
            k = re.search(r"\d+(search_kernel|scores_kernel|counts_kernel)", m.group(1))
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
    ap.add_argument("--unique", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--network", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        res["device"] = torch.cuda.get_device_name(0)
        res["run"] = run(a.frames, a.unique, a.repeats, a.window, torch.device("cuda:0"), a.network)
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
