"""Device time of the tracking solve (df3d_track_peaks) in ms per 1 000 frames at T = 1 000, 12 500 and 100 000
frames of 133 chains with K = 10 peaks, at block_frames 256 and 4 096.  Timed with device events round the C entry alone (workspace
allocated once, outside the window), after two warm-ups, over as many calls as fill half a second.  --peaks also times the stage that
feeds it, df3d_heatmap_peaks, on 7 x 100 frames of random heat-maps, and reports the ratio; DESIGN.md section 9 has that stage at 11.0 ms
per 1 000 frames.  --resources compiles the file once more with the compiler's resource report; --resources-only needs no device.  The
numbers gate nothing.

    python tests/perf/bench_track.py [--frames 1000 12500 100000] [--blocks 256 4096] [--peaks] [--resources] [--out result.json]
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

C, J, K = 7, 19, 10
IMAGE_SHAPE = [960, 480]


def peaks(T, dev, seed=31):
    """count [7, T, 19] int32, pts [7, T, 19, K, 2] and val [7, T, 19, K] float32 on the device: K peaks on heat-map cells, values falling
    with the slot as df3d_heatmap_peaks sorts them, a twentieth of the frames with fewer peaks."""
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    count = torch.full((C, T, J), K, dtype=torch.int32, device=dev)
    few = torch.rand((C, T, J), generator=g, device=dev) < 0.05
    count[few] = torch.randint(0, K, (int(few.sum()),), generator=g, device=dev, dtype=torch.int32)
    cell = torch.stack([torch.randint(0, 64, (C, T, J, K), generator=g, device=dev), torch.randint(0, 128, (C, T, J, K), generator=g, device=dev)], dim=-1)
    pts = (cell.to(torch.float32) / torch.tensor([64.0, 128.0], device=dev)).contiguous()
    val = torch.sort(torch.rand((C, T, J, K), generator=g, device=dev), dim=-1, descending=True).values.contiguous()
    return count, pts, val


def timed(fn, window_s=0.5, warmup=2, most=400):
    import torch

    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    reps = int(min(most, max(3, window_s * 1e3 / max(start.elapsed_time(stop), 1e-3))))
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps, reps   # ms per call


def run(T, blocks, dev):
    import torch

    from deepfly3d_amd import _native

    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    count, pts, val = peaks(T, dev)
    choice = torch.empty((C, T, J), dtype=torch.int32, device=dev)
    cost = torch.empty((C, J), dtype=torch.int64, device=dev)
    res = {"frames": T, "chains": C * J, "K": K, "blocks": {}}
    first = None
    for block in blocks:
        need = lib.df3d_track_work_bytes(C * J, T, K, block)
        work = torch.empty((need,), dtype=torch.uint8, device=dev)

        def call():
            _native.check(lib.df3d_track_peaks(count.data_ptr(), pts.data_ptr(), val.data_ptr(), C, T, J, K, float(IMAGE_SHAPE[1]), float(IMAGE_SHAPE[0]),
                                               30.0, 1.0, 1.0, block, choice.data_ptr(), cost.data_ptr(), work.data_ptr(), need, stream), "df3d_track_peaks")

        ms, reps = timed(call)
        if first is None:
            first = (choice.clone(), cost.clone())
        same = bool(torch.equal(first[0], choice) and torch.equal(first[1], cost))   # blocking changes no bit
        res["blocks"][str(block)] = {"ms_per_call": ms, "ms_per_1000_frames": ms * 1000.0 / T, "calls": reps, "work_bytes": need,
                                     "time_blocks": -(-T // block), "same_bits_as_first": same}
        del work
    res["off_slot_0"] = float((choice != 0).float().mean())
    return res


def peaks_stage(dev, frames=100):
    """ms per 1 000 frames of df3d_heatmap_peaks at K = 10 on 7 x `frames` x 19 random heat-maps (64 x 128)."""
    import torch

    from deepfly3d_amd import ops

    g = torch.Generator(device=dev).manual_seed(5)
    hm = torch.rand((C * frames, J, 64, 128), generator=g, device=dev)
    ms, reps = timed(lambda: ops.heatmap_peaks(hm, K))
    return {"frames": frames, "ms_per_call": ms, "ms_per_1000_frames": ms * 1000.0 / frames, "calls": reps}


def resources():
    """name -> {vgprs, agprs, sgprs, lds_bytes, scratch_bytes, waves_per_simd} from the compiler's resource report of the file."""
    from deepfly3d_amd import build

    src = os.path.join(ROOT, "deepfly3d_amd", "csrc", "track.hip")
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
            k = re.search(r"\d+(track_\w+?_kernel)(ILb([01]))?", m.group(1))
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
    ap.add_argument("--frames", type=int, nargs="+", default=[1000, 12500, 100000])
    ap.add_argument("--blocks", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--peaks", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--resources-only", dest="resources_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.resources_only:
        import torch

        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        res["runs"] = [run(T, a.blocks, dev) for T in a.frames]
        if a.peaks:
            res["heatmap_peaks"] = peaks_stage(dev)
            for r in res["runs"]:
                for b in r["blocks"].values():
                    b["ratio_to_heatmap_peaks"] = b["ms_per_1000_frames"] / res["heatmap_peaks"]["ms_per_1000_frames"]
    if a.resources or a.resources_only:
        res["resources"] = resources()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
