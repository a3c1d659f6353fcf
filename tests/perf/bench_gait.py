"""Device time of every entry of the gait analysis at T = 100 000 and 8 192 frames, timed with device events (5
calls after 2 warm-ups), each beside a byte model at 8 TB/s: every operand read once and every result written once, a scanned
series of T int32 read twice and written once (block results, apply) after the kernel that wrote it.  The entries are chains of short
launches (the steps: 13), so at these sizes the launches, not the bytes, set the time: the fraction says how far from the memory
system's limit a recording of this length sits, nothing more.  --resources compiles the file once more with the compiler's
resource report and lists VGPRs, SGPRs, LDS, scratch and waves per SIMD of every kernel; --resources-only needs no device.  The
numbers gate nothing.

    python tests/perf/bench_gait.py [--frames 100000 8192] [--resources] [--out result.json]
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

HBM = 8e12   # bytes per second
TIPS = [4, 9, 14, 23, 28, 33]
COXAE = [0, 5, 10, 19, 24, 29]


def walker(T, seed=29):
    """[T, 38, 3]: a pose whose body frame is close to the world's axes and that trembles a little, every tip on a rhythm of its own
    along x (10 to 21 units per second at 100 fps: past the default thresholds), a hundredth of the frames with a missing tip."""
    rng = np.random.default_rng(seed)
    pose = rng.normal(0.0, 1.0, (38, 3))
    pose[COXAE] = [[x, side * y, z] for side in (1.0, -1.0) for x, y, z in ((0.6, 0.35, 0.1), (0.0, 0.45, 0.0), (-0.7, 0.4, 0.1))]
    X = pose[None] + rng.normal(0.0, 0.002, (T, 38, 3))
    X[:, TIPS, 0] += 0.5 * np.sin(np.arange(T)[:, None] * (2 * np.pi / rng.uniform(15.0, 30.0, 6)) + rng.uniform(0.0, 6.0, 6))
    for leg in range(6):
        X[rng.random(T) < 0.01 / 6, TIPS[leg]] = 0.0
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


def run(T, dev):
    import torch

    from deepfly3d_amd import _native, config, ops

    lib, check = _native.load(), _native.check
    stream = torch.cuda.current_stream(dev).cuda_stream
    X = torch.from_numpy(walker(T)).to(dev)
    frame = ops.recording_frame(X)
    fps, on, off, w = 100.0, config.GAIT_SWING_ON, config.GAIT_SWING_OFF, config.GAIT_DIFF_HALF
    need = lib.df3d_gait_work_bytes(T)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    tip, vel, phase, mean, metrics = f64(T, 6, 3), f64(T, 6, 3), f64(T, 6), f64(6, 6, 2), f64(3 * T, 3)
    states, pattern, count = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((T, 6), (T,), (1,)))
    steps, pairs, hist, counts = (torch.empty(s, dtype=torch.int64, device=dev) for s in ((3 * T, 4), (6, 6), (64,), (6, 3)))
    res = {"frames": T, "work_bytes": need}
    blocks = (T + 255) // 256

    def entry(name, fn, nbytes, **more):
        us = timed(fn)
        res[name] = {"us": us, "bytes": nbytes, "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM, **more}

    scan = lambda rows: rows * (T * 12 + blocks * 12)   # noqa: E731  (block results: read T, write nb; carry: nb twice; apply: read T and nb, write T)
    events = T * 6 * (8 + 16) + scan(24)                # the states and their neighbour read, four series written, then scanned
    entry("velocity", lambda: check(lib.df3d_gait_velocity(X.data_ptr(), T, frame.data_ptr(), 1, fps, w, tip.data_ptr(), vel.data_ptr(), stream)),
          T * 6 * (4 * 24 + 48), launches=1)   # P0 and P4 of t, P4 of a and b; tip and vel
    entry("states (codes + max-scan + states)",
          lambda: check(lib.df3d_gait_states(vel.data_ptr(), T, on, off, states.data_ptr(), work.data_ptr(), need, stream)),
          T * 6 * (8 + 4) + scan(6) + T * 6 * (4 + 8 + 4), launches=5)
    entry("steps (events + max-scan + flags + sum-scan + rows)",
          lambda: check(lib.df3d_gait_steps(states.data_ptr(), tip.data_ptr(), T, fps, steps.data_ptr(), metrics.data_ptr(), count.data_ptr(),
                                            work.data_ptr(), need, stream)),
          events + T * 6 * (12 + 4) + T * 6 * 12 + 3 * T * 56 + T * 6 * 8, launches=13)
    res["steps (events + max-scan + flags + sum-scan + rows)"]["steps"] = int(count.item())
    entry("phase (events + max-scan + phase)", lambda: check(lib.df3d_gait_phase(states.data_ptr(), T, phase.data_ptr(), work.data_ptr(), need, stream)),
          events + T * 6 * (12 + 8), launches=5)
    entry("coupling (slices + fold)",
          lambda: check(lib.df3d_gait_coupling(phase.data_ptr(), T, mean.data_ptr(), pairs.data_ptr(), work.data_ptr(), need, stream)),
          T * 48 + 2 * ((T + 2047) // 2048) * 864, launches=2, slices=(T + 2047) // 2048, sincos=6 * T)
    entry("patterns", lambda: check(lib.df3d_gait_patterns(states.data_ptr(), T, pattern.data_ptr(), hist.data_ptr(), counts.data_ptr(), stream)),
          T * 28, launches=3)
    res["ops.gait (with its read-back of S and allocations)"] = {"us": timed(lambda: ops.gait(X, fps, frame))}
    return res


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "gait.hip")
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
            k = re.search(r"\d+(gait_\w+?_kernel)", m.group(1))
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
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        res["runs"] = [run(T, dev) for T in a.frames]
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
