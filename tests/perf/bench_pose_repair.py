"""Device time of the pose repair at T = 8 192 and 100 000 frames and half windows of 5 and 64, timed with
device events (5 calls after 2 warm-ups): df3d_repair_outliers, df3d_repair_fill and ops.repair_pose (with its allocations).  Each
beside a model.  The fill: every operand read once and every result written once at 8 TB/s, a scanned series of T int32 read twice
and written once after the kernel that wrote it.  The outlier test: its LDS reads -- rank counting reads the window once per
candidate, for the values and for the deviations of three coordinates, 6 W^2 eight-byte reads per tested joint at most (a lane
stops at the candidate that completes the pair of middle ranks) -- against 256 bytes per clock and CU.  --resources compiles the
file once more with the compiler's resource report and lists VGPRs, SGPRs, LDS, scratch and waves per SIMD of every kernel;
--resources-only needs no device.  The numbers gate nothing.

    python tests/perf/bench_pose_repair.py [--frames 8192 100000] [--half 5 64] [--resources] [--out result.json]
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

HBM = 8e12            # bytes per second
LDS_PER_CLK_CU = 256  # bytes: ds_read_b64 over 64 lanes in two clocks


def recording(T, seed=31):
    """[T, 38, 3]: a pose that trembles, every joint on a slow rhythm of its own, one joint in a hundred missing (in runs of one to
    twelve frames) and one in a thousand a spike."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None]
    X = rng.normal(0.0, 1.0, (1, 38, 3)) + 0.5 * np.sin(t * (2 * np.pi / rng.uniform(15.0, 40.0, (1, 38, 3)))) + rng.normal(0.0, 0.005, (T, 38, 3))
    spikes = rng.random((T, 38)) < 1e-3
    X[spikes] += rng.choice([-3.0, 3.0], size=(int(spikes.sum()), 1))
    for s, j in zip(rng.integers(0, T, size=T * 38 // 600), rng.integers(0, 38, size=T * 38 // 600)):
        X[s:s + int(rng.integers(1, 13)), j] = 0.0
    return X


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


def run(T, h, dev):
    import torch

    from deepfly3d_amd import _native, config, ops

    lib, check = _native.load(), _native.check
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(dev)
    cus, clock = props.multi_processor_count, getattr(props, "clock_rate", 2400000) * 1e3   # Hz
    X = torch.from_numpy(recording(T)).to(dev)
    scale = config.REPAIR_THRESHOLD * config.REPAIR_MAD_TO_SIGMA
    need = lib.df3d_repair_work_bytes(T)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    flags = torch.empty((T, 38), dtype=torch.uint8, device=dev)
    score, out = torch.empty((T, 38), dtype=torch.float64, device=dev), torch.empty((T, 38, 3), dtype=torch.float64, device=dev)
    status, counts = torch.empty((T, 38), dtype=torch.int8, device=dev), torch.empty((38, 5), dtype=torch.int64, device=dev)
    res = {"frames": T, "half_window": h, "work_bytes": need, "compute_units": cus, "clock_hz": clock}
    W, blocks = 2 * h + 1, (T + 255) // 256
    us = timed(lambda: check(lib.df3d_repair_outliers(X.data_ptr(), T, h, scale, config.REPAIR_FLOOR, config.REPAIR_MIN_COUNT, flags.data_ptr(),
                                                      score.data_ptr(), stream)))
    reads = 6 * W * W * T * 38
    model_us = reads * 8 / (LDS_PER_CLK_CU * cus * clock) * 1e6
    res["outliers"] = {"us": us, "lds_reads": reads, "model_us": model_us, "fraction_of_lds_model": model_us / us,
                       "bytes": T * 38 * (24 + 1 + 8), "launches": 1}
    tested = int((flags == 0).sum() + (flags == 2).sum())
    res["outliers"]["outliers"], res["outliers"]["missing"], res["outliers"]["not_missing"] = int((flags == 2).sum()), int((flags == 1).sum()), tested
    # good: flags read, two series written; scan: T read twice and written once per row, block results; fill: points, flags read, out, status written
    nbytes = T * 38 * (1 + 8) + 76 * (T * 12 + blocks * 12) + T * 38 * (24 + 1 + 24 + 1)
    us = timed(lambda: check(lib.df3d_repair_fill(X.data_ptr(), flags.data_ptr(), T, config.REPAIR_MAX_GAP, out.data_ptr(), status.data_ptr(),
                                                  counts.data_ptr(), work.data_ptr(), need, stream)))
    res["fill (good + max-scan + fill)"] = {"us": us, "bytes": nbytes, "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM, "launches": 6,
                                            "codes": counts.sum(dim=0).tolist()}
    res["ops.repair_pose (with its allocations)"] = {"us": timed(lambda: ops.repair_pose(X, half_window=h))}
    return res


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "pose_repair.hip")
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
            k = re.search(r"\d+(repair_\w+?_kernel)", m.group(1))
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
    ap.add_argument("--frames", type=int, nargs="+", default=[8192, 100000])
    ap.add_argument("--half", type=int, nargs="+", default=[5, 64])
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        res["runs"] = [run(T, h, dev) for T in a.frames for h in a.half]
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
