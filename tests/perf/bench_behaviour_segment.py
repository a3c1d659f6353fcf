"""Device time of every entry of the behaviour map's segmentation at T = 100 000 and 8 192 frames on a grid of
G = 256, timed with device events (5 calls after 2 warm-ups).  The density is set beside the float64 matrix peak on the model
2 G^2 T flop (the product) and beside the count of its exponentials, 2 G T per tile column or row, that is 2 G T (G / 64) in all; the
integer entries beside a byte model (every operand read once, every result written once; a jump round reads two and writes one
int32 per cell) at 8 TB/s.  --resources compiles the file once more with the compiler's resource report and lists VGPRs, AGPRs, LDS
and waves per SIMD of every kernel; --resources-only needs no device.  The numbers gate nothing.

    python tests/perf/bench_behaviour_segment.py [--frames 100000 8192] [--grid 256] [--resources] [--out result.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM = 8e12               # bytes per second
FP64_MATRIX = 78.6e12    # flop per second
TILE = 64


def cloud(T, seed=23):
    """[T, 2]: a map of eight clumps and a thin background, a hundredth of the rows without a place."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-40.0, 40.0, size=(8, 2))
    Y = centres[rng.integers(0, 8, size=T)] + rng.standard_normal((T, 2)) * np.where(rng.random((T, 1)) < 0.1, 12.0, 3.0)
    Y[rng.random(T) < 0.01] = np.nan
    return Y


def timed(fn, warmup=2, reps=5):
    import torch

    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps   # us per call


def run(T, G, dev):
    import torch

    from deepfly3d_amd import _native, config, ops

    lib, check = _native.load(), _native.check
    stream = torch.cuda.current_stream(dev).cuda_stream
    Y = torch.from_numpy(cloud(T)).to(dev)
    n = G * G
    need = lib.df3d_bseg_work_bytes(T, G)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    bounds = torch.empty((5,), dtype=torch.float64, device=dev)
    rho = torch.empty((G, G), dtype=torch.float64, device=dev)
    regions, roots = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    count, nbouts = torch.empty((1,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
    labels = torch.empty((T,), dtype=torch.int32, device=dev)
    bouts = torch.empty((T, 3), dtype=torch.int64, device=dev)
    res = {"frames": T, "grid": G, "work_bytes": need}

    us = timed(lambda: check(lib.df3d_bseg_bounds(Y.data_ptr(), T, bounds.data_ptr(), stream)))
    res["bounds (one block)"] = {"us": us, "bytes": T * 16, "fraction_of_8TBps": T * 16 / (us * 1e-6) / HBM}
    b = bounds.cpu().tolist()
    (x0, y0, h), sigma = ops.density_grid((b[0], b[2]), (b[1], b[3]), G)
    us = timed(lambda: check(lib.df3d_bseg_density(Y.data_ptr(), T, x0, y0, h, G, sigma, rho.data_ptr(), work.data_ptr(), need, stream)))
    flop, exps = 2.0 * n * T, 2.0 * G * T * ((G + TILE - 1) // TILE)
    res["density (bounds + product + fold)"] = {"us": us, "flop": flop, "fraction_of_fp64_matrix_peak": flop / (us * 1e-6) / FP64_MATRIX,
                                               "exponentials": exps, "exponentials_per_us": exps / us,
                                               "slices": (T + 2047) // 2048, "blocks": ((G + TILE - 1) // TILE) ** 2 * ((T + 2047) // 2048)}
    us = timed(lambda: check(lib.df3d_bseg_watershed(rho.data_ptr(), G, config.BEHAVIOUR_MIN_PEAK, regions.data_ptr(), count.data_ptr(), roots.data_ptr(),
                                                     work.data_ptr(), need, stream)))
    rounds = int(np.ceil(np.log2(n)))
    nbytes = n * (8 + 8 * 9 + 4) + rounds * n * 12 + n * (8 + 4 + 4) + 3 * n * 8 + n * 20   # max, ascent, jumps, keep, scan, regions
    res["watershed (max + ascent + jumps + scan + regions)"] = {"us": us, "jump_rounds": rounds, "launches": 7 + rounds, "bytes": nbytes,
                                                               "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM, "regions": int(count.item())}
    us = timed(lambda: check(lib.df3d_bseg_labels(Y.data_ptr(), T, x0, y0, h, G, regions.data_ptr(), labels.data_ptr(), stream)))
    res["labels"] = {"us": us, "bytes": T * 24, "fraction_of_8TBps": T * 24 / (us * 1e-6) / HBM}
    R = int(count.item())
    occ = torch.empty((R + 1,), dtype=torch.int64, device=dev)
    tr = torch.empty((R + 1, R + 1), dtype=torch.int64, device=dev)
    us = timed(lambda: check(lib.df3d_bseg_bouts(labels.data_ptr(), T, R, bouts.data_ptr(), nbouts.data_ptr(), occ.data_ptr(), tr.data_ptr(),
                                                 work.data_ptr(), need, stream)))
    nbytes = T * (8 + 3 * 8 + 12 + 4 + 24 + 8) + (R + 1) * (R + 2) * 8   # starts, scan, bout starts, bouts, counts, the two tables
    res["bouts (starts + scan + bouts + counts)"] = {"us": us, "launches": 9, "bytes": nbytes, "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM,
                                                    "bouts": int(nbouts.item())}
    us = timed(lambda: ops.segment_map(Y, G))
    res["ops.segment_map (with its three read-backs and allocations)"] = {"us": us}
    return res


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "behaviour_segment.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", os.path.join(tmp, "x.o"),
               "-Rpass-analysis=kernel-resource-usage"]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=tmp).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes", "ScratchSize [bytes/lane]": "scratch_bytes",
            "Occupancy [waves/SIMD]": "waves_per_simd"}
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"\d+(bseg_\w+?_kernel)", m.group(1))
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
    ap.add_argument("--frames", type=int, nargs="+", default=[100000, 8192])
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        res["runs"] = [run(T, a.grid, dev) for T in a.frames]
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
