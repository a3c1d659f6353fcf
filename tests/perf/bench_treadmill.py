"""Device time of every entry of the treadmill analysis at T = 100 000 and 8 192 frames, timed with device
events (5 calls after 2 warm-ups), each beside a byte model at 8 TB/s: every operand read once per launch that reads it and every
result written once.  The entries are chains of short launches (the known-radius fit: 22), so at these sizes the launches, not the
bytes, set the time: the fraction says how far from the memory system's limit a recording of this length sits, nothing more.
--resources compiles the file once more with the compiler's resource report and lists VGPRs, SGPRs, LDS, scratch and waves per SIMD of
every kernel; --resources-only needs no device.  The numbers gate nothing.

    python tests/perf/bench_treadmill.py [--frames 100000 8192] [--resources] [--out result.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_gait import HBM, timed, walker  # noqa: E402


def run(T, dev):
    import torch

    from deepfly3d_amd import _native, config, ops

    lib, check = _native.load(), _native.check
    stream = torch.cuda.current_stream(dev).cuda_stream
    X = torch.from_numpy(walker(T)).to(dev)
    frame = ops.recording_frame(X).reshape(3, 3).contiguous()
    coxa = ops._coxa_medians(X)[1].contiguous()
    fps, w = 100.0, config.GAIT_DIFF_HALF
    need = lib.df3d_ball_work_bytes(T)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    tip, vel, ball, sums, omega, residual, fictive, path = f64(T, 6, 3), f64(T, 6, 3), f64(8), f64(17), f64(T, 3), f64(T), f64(T, 3), f64(T, 3)
    legs = torch.empty((T,), dtype=torch.int32, device=dev)
    info, skipped = torch.empty((2,), dtype=torch.int64, device=dev), torch.empty((1,), dtype=torch.int64, device=dev)
    res = {"frames": T, "work_bytes": need}
    slices, blocks = (6 * T + 2047) // 2048, (T + 255) // 256

    def entry(name, fn, nbytes, **more):
        us = timed(fn)
        res[name] = {"us": us, "bytes": nbytes, "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM, **more}

    entry("tips", lambda: check(lib.df3d_ball_tips(X.data_ptr(), T, frame.data_ptr(), coxa.data_ptr(), fps, w, tip.data_ptr(), vel.data_ptr(), stream)),
          T * 6 * (3 * 24 + 48), launches=1)   # P4 of t, a and b; tip and vel
    states = ops.gait_states(vel)
    sweep = T * 6 * 28 + 2 * slices * 128   # one pass over tips and states, its partials written and folded
    pivot = float(config.BALL_PIVOT_MIN)
    for name, known, passes in (("fit, free radius (3 sum passes + solves)", 0, 3),
                                (f"fit, known radius ({config.BALL_FIT_ITERATIONS} steps: {3 + config.BALL_FIT_ITERATIONS} sum passes + solves)", 1,
                                 3 + config.BALL_FIT_ITERATIONS)):
        entry(name, lambda known=known: check(lib.df3d_ball_fit(tip.data_ptr(), states.data_ptr(), T, known, 4.0, config.BALL_FIT_ITERATIONS, pivot,
                                                                ball.data_ptr(), info.data_ptr(), sums.data_ptr(), work.data_ptr(), need, stream)),
              passes * sweep, launches=2 * passes, slices=slices)
    res["ball"] = {"center_radius_rms": ball.cpu().tolist()[:5], "count_status": info.cpu().tolist()}
    entry("rotation", lambda: check(lib.df3d_ball_rotation(tip.data_ptr(), vel.data_ptr(), states.data_ptr(), T, ball.data_ptr(), config.BALL_MIN_LEGS,
                                                           float(config.BALL_FRAME_PIVOT_MIN), omega.data_ptr(), legs.data_ptr(), residual.data_ptr(),
                                                           fictive.data_ptr(), stream)),
          T * (6 * 52 + 24 + 4 + 8 + 24), launches=1)
    entry("path (two scans of three launches)", lambda: check(lib.df3d_ball_path(fictive.data_ptr(), T, fps, path.data_ptr(), skipped.data_ptr(),
                                                                                  work.data_ptr(), need, stream)),
          T * (2 * 24 + 8) + 2 * T * (2 * 32 + 8) + 3 * blocks * 24, launches=7, sincos=4 * T)
    res["skipped"] = int(skipped.item())
    res["ops.treadmill (with gait_states, the medians, the frame and its allocations)"] = {"us": timed(lambda: ops.treadmill(X, fps))}
    return res


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "treadmill.hip")
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
            k = re.search(r"\d+((?:ball|path)_\w+?_kernel)(ILi(\d)E)?", m.group(1))
            name = (k.group(1) + (f"<{k.group(3)}>" if k.group(2) else "")) if k else None
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
