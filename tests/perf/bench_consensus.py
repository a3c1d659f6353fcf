"""Device time of the consensus triangulation (df3d_triangulate_consensus) against df3d_triangulate on the same
input: 1 000 frames x 38 joints at the fly layout (7 cameras, the visibility of config.camera_see_joint: 2 to 4 views a joint) and with
8 views everywhere (247 candidates a point).  Both entries are timed with device events round the C entry alone (outputs and workspace
allocated once, outside the window), after warm-ups, in --repeats windows of --window seconds each, the two entries alternating; the
median, the smallest and the largest window are reported.  The float64 share is the operations the algorithm needs (counted here from
the shapes, with the Jacobi sweeps of every candidate counted by a numpy run of the same cyclic scheme; a division and a square root
count as one operation each, though the device expands them) over the median time, over the 78.6 Tflop/s float64 vector peak.
--resources compiles the file once more with the compiler's resource report; --resources-only needs no device.  The numbers gate
nothing.

    python tests/perf/bench_consensus.py [--frames 1000] [--repeats 5] [--window 0.3] [--resources] [--out result.json]
"""
import argparse
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
FP64_PEAK = 78.6e12
ROTATION_FLOPS = 53    # theta 3, t 5, c 4, s 1, the two diagonal entries 4, the two other rows 12, the eigenvectors 24
ERROR_FLOPS = 26       # projection 18, two divisions, two differences, the sum of two squares 3, the square root


def inputs(layout, T):
    """(P [ncam, 3, 4], px [ncam, T, 38, 2]) of a layout: "fly" or "eight"."""
    import consensus_cases as cc

    if layout == "fly":
        return cc.rig(7), cc.fly_layout(T)[0]
    return cc.rig(8), _eight(T)


def _eight(T):
    """Eight views everywhere, an outlier planted in one view of every fifth point."""
    import consensus_cases as cc
    import pose_chain_cases as pc

    px = pc.detections(pc.TRI_SEED + 21, T * J)[0][:, :, 0].copy()
    rng = np.random.default_rng(21)
    for i in range(0, T * J, 5):
        a = rng.uniform(0.0, 2.0 * np.pi)
        px[int(rng.integers(8)), i] += cc.OUTLIER_PX * np.array([np.sin(a), np.cos(a)])
    return np.ascontiguousarray(px.reshape(8, T, J, 2))


def jacobi_sweeps(M):
    """Sweeps of the cyclic Jacobi scheme of csrc/geometry_dev.h on M [N, 4, 4] (symmetric, scaled by 1 / trace), per matrix."""
    a = M / np.trace(M, axis1=1, axis2=2)[:, None, None]
    sweeps = np.zeros(len(a), dtype=np.int64)
    iu = np.triu_indices(4, 1)
    for _ in range(16):
        live = np.abs(a[:, iu[0], iu[1]]).sum(axis=1) >= 1e-40
        if not live.any():
            break
        sweeps += live
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            apq = a[:, p, q]
            on = live & (np.abs(apq) > 1e-300)
            with np.errstate(all="ignore"):
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(on, t, 0.0)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            R = np.broadcast_to(np.eye(4), a.shape).copy()
            R[:, p, p], R[:, q, q], R[:, p, q], R[:, q, p] = c, c, s, -s
            a = np.einsum("nji,njk,nkl->nil", R, a, R)
    return sweeps


SAMPLE = 1900   # points the operations are counted on (50 frames), scaled to the input


def flops(P, px):
    """The float64 operations the fused entry needs on this input and the candidates it forms, counted on the first SAMPLE points and
    scaled."""
    import consensus_oracle as co

    ncam = px.shape[0]
    flat = px.reshape(ncam, -1, 2)
    scale = flat.shape[1] / min(flat.shape[1], SAMPLE)
    flat = flat[:, :SAMPLE]
    vis = (flat != 0.0).all(axis=-1)
    r0 = flat[..., 1:2] * P[:, None, 2, :] - P[:, None, 0, :]
    r1 = flat[..., 0:1] * P[:, None, 2, :] - P[:, None, 1, :]
    C = (r0[..., :, None] * r0[..., None, :] + r1[..., :, None] * r1[..., None, :]) * vis[..., None, None]   # [ncam, N, 4, 4]
    vm = (vis * (1 << np.arange(ncam))[:, None]).sum(axis=0)
    total, candidates = 31.0 * vis.sum(), 0     # a view's contribution: 8 + 30, less the 7 entries below the diagonal
    for mask in range(1 << ncam):
        cams = co.cams_of(mask)
        at = np.nonzero(((vm & mask) == mask) & (vm != mask))[0] if len(cams) >= 2 else ()
        if len(at):
            sweeps = jacobi_sweeps(C[cams][:, at].sum(axis=0))
            total += float((10 * len(cams) + 14 + 3 + sweeps * (6 * ROTATION_FLOPS + 5)).sum()) + len(at) * len(cams) * (ERROR_FLOPS + 1)
            candidates += len(at)
    n = vis.sum(axis=0)
    total += float((n[n >= 2] * 2 * (ERROR_FLOPS + 1)).sum())    # the all-views candidate and the chosen point's errors
    return total * scale, int(round((candidates + int((n >= 2).sum())) * scale))


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


def run(layout, T, repeats, window_s, dev):
    import ctypes

    import torch

    from deepfly3d_amd import _native, config

    lib = _native.load()
    P, px = inputs(layout, T)
    ncam = px.shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    d = torch.from_numpy(px).to(dev)
    full = torch.empty((T, J, 3), dtype=torch.float64, device=dev)
    X = torch.empty_like(full)
    cameras = torch.empty((T, J), dtype=torch.int32, device=dev)
    status = torch.empty((T, J), dtype=torch.int8, device=dev)
    err = torch.empty((ncam, T, J), dtype=torch.float64, device=dev)
    fixed = torch.empty((ncam, T, J, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((J, 4), dtype=torch.int64, device=dev)
    need = lib.df3d_consensus_work_bytes(ncam, T, J)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    tau = np.ascontiguousarray(config.ROBUST_TAU)
    dp = ctypes.POINTER(ctypes.c_double)

    def plain():
        _native.check(lib.df3d_triangulate(P.ctypes.data_as(ctypes.c_void_p), d.data_ptr(), ncam, T, J, full.data_ptr(), stream), "df3d_triangulate")

    def fused():
        _native.check(lib.df3d_triangulate_consensus(P.ctypes.data_as(dp), d.data_ptr(), full.data_ptr(), ncam, T, J, tau.ctypes.data_as(dp), 2, X.data_ptr(),
                                                     cameras.data_ptr(), status.data_ptr(), err.data_ptr(), fixed.data_ptr(), counts.data_ptr(),
                                                     work.data_ptr(), need, stream), "df3d_triangulate_consensus")

    plain()
    (t_plain, t_fused), reps = windows((plain, fused), repeats, window_s)
    ops, candidates = flops(P, px)

    def spread(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}

    med = statistics.median(t_fused)
    return {"layout": layout, "ncam": ncam, "frames": T, "joints": J, "candidates": candidates, "calls_per_window": reps, "windows": repeats,
            "df3d_triangulate": spread(t_plain), "df3d_triangulate_consensus": spread(t_fused),
            "ratio_of_medians": med / statistics.median(t_plain), "fp64_operations": ops, "fp64_tflops": ops / (med * 1e-3) / 1e12,
            "fp64_share_of_peak": ops / (med * 1e-3) / FP64_PEAK, "status_counts": counts.sum(dim=0).tolist()}


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd, sgpr_spills, vgpr_spills} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "consensus.hip")
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
            k = re.search(r"\d+((?:consensus|count_\w+?)_kernel)(ILb([01]))?", m.group(1))
            name = (k.group(1) + ("<true>" if k.group(3) == "1" else "<false>" if k.group(3) == "0" else "")) if k else None
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
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        res["runs"] = [run(layout, a.frames, a.repeats, a.window, dev) for layout in ("fly", "eight")]
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
