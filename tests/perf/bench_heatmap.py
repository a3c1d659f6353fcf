"""Device time of the heat-map overlay and the rate of the heat-map video loop.

1. The drawing launch (df3d_render_heatmap) at the video frame's shape, 6 views x 480 x 960 over 19 planes of 64 x 128 each, beside
   the pose-2d frame's launch (df3d_render_pose2d_grid) on the same images: alternating windows of --launches launches round device
   events after a warm-up window of each; median and spread over --rounds windows, and the time the bytes model allows (each input
   read once, the frame written once, at the HBM peak) beside it.
2. The video loops on a folder of camera images: frames/s of video.make_heatmap_video against video.make_pose2d_video on the same
   folder and the same detections (host clock round the whole call, which ends with the encoder closed: file reads, device JPEG
   decode, the network for the heat-map video, drawing, the copy to the host and the encoder).  Needs weights ($DF3D_WEIGHTS or
   DF3D_SYNTHETIC_WEIGHTS=<seed>) and a folder (--folder; default: the golden sample images, --frames of them by repeating them).

    python tests/perf/bench_heatmap.py [--rounds 21] [--launches 200] [--frames 64] [--folder DIR] [--out result.txt]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import ops, video  # noqa: E402
from deepfly3d_amd.config import camera_is_flipped, config, heatmap_planes, plane_color  # noqa: E402

HBM = 8e12   # bytes per second
S, H, W, P, HH, WH = 6, 480, 960, 19, 64, 128


def bytes_model(nsel):
    """Bytes one launch has to move: the six images, the selected planes once each (the taps of neighbouring pixels hit the caches),
    the RGB frame."""
    return {"luma": S * H * W, "heatmaps": sum(nsel) * HH * WH * 4, "frame": S * H * W * 3}


def window(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches   # us per launch


def stats(v):
    v = np.asarray(v)
    med = float(np.median(v))
    return {"median_us": med, "min_us": float(v.min()), "max_us": float(v.max()), "spread": float((v.max() - v.min()) / med)}


def drawing(dev, rounds, launches):
    g = torch.Generator(device=dev).manual_seed(0)
    luma = torch.randint(0, 256, (S, H, W), dtype=torch.uint8, device=dev, generator=g)
    # Gaussian blobs of sigma 1.5 cells, one per plane: what the network's maps look like
    cr = torch.rand((S, P, 1, 1), generator=g, device=dev) * (HH - 7) + 3
    cc = torch.rand((S, P, 1, 1), generator=g, device=dev) * (WH - 7) + 3
    r, c = torch.arange(HH, device=dev).view(1, 1, HH, 1), torch.arange(WH, device=dev).view(1, 1, 1, WH)
    hm = torch.exp(-((r - cr) ** 2 + (c - cc) ** 2) / (2.0 * 1.5 * 1.5)).float().contiguous()
    pairs = [heatmap_planes(cam) for cam in video.GRID_CAMERAS]
    planes, colors = [[p for p, _ in pr] for pr in pairs], [[plane_color(j) for _, j in pr] for pr in pairs]
    flips = [camera_is_flipped(cam) for cam in video.GRID_CAMERAS]
    out = torch.empty((2 * H, 3 * W, 3), dtype=torch.uint8, device=dev)
    renderer = video.FrameRenderer(H, W, config["num_joints"], dev)
    pts = (torch.rand((S, config["num_joints"], 2), generator=g, device=dev, dtype=torch.float64) * torch.tensor([H, W], device=dev)).contiguous()
    out2 = torch.empty_like(out)

    def heat():
        ops.render_heatmap(luma, hm, planes, colors, flips, cols=3, out=out)

    def pose():
        renderer.grid2d(luma, pts, out=out2)

    for fn in (heat, pose):   # warm-up: code objects loaded, clocks up
        window(fn, launches)
    t = {"heatmap": [], "pose2d": []}
    for _ in range(rounds):   # alternating windows: both kernels see the same neighbours on the machine
        t["heatmap"].append(window(heat, launches))
        t["pose2d"].append(window(pose, launches))
    model = bytes_model([len(p) for p in planes])
    total = sum(model.values())
    res = {"shape": [S, H, W], "planes_selected": [len(p) for p in planes], "bytes_model": model, "bytes_total": total, "us_at_8TBps": total / HBM * 1e6,
           "heatmap": stats(t["heatmap"]), "pose2d": stats(t["pose2d"])}
    res["heatmap"]["fraction_of_8TBps"] = total / (res["heatmap"]["median_us"] * 1e-6) / HBM
    res["ratio_heatmap_over_pose2d"] = res["heatmap"]["median_us"] / res["pose2d"]["median_us"]
    return res


def sample_folder(frames, root):
    """`frames` images per camera in a fresh folder: the golden sample frames, repeated."""
    src = os.path.join(ROOT, "tests", "golden", "images")
    have = sorted({int(f.split("_img_")[1].split(".")[0]) for f in os.listdir(src) if f.startswith("camera_0_img_")})
    folder = os.path.join(root, "images")
    os.makedirs(folder)
    for t in range(frames):
        for cam in range(config["num_cameras"]):
            shutil.copy(os.path.join(src, f"camera_{cam}_img_{have[t % len(have)]}.jpg"), os.path.join(folder, f"camera_{cam}_img_{t}.jpg"))
    return folder


def loops(folder, repeats):
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    core = Core(folder, None, 0)
    core.pose2d_estimation()
    core.calibrate_calc(0, core.max_img_id)
    res = {"frames": core.num_images, "encoder": "ffmpeg" if shutil.which("ffmpeg") else "mjpeg-avi", "dtype": core.dtype}
    makers = {"heatmap": video.make_heatmap_video, "pose2d": video.make_pose2d_video}
    for fn in makers.values():   # warm-up: engine built, code objects loaded, files in the page cache
        fn(core, fps=30)
    t = {k: [] for k in makers}
    for _ in range(repeats):     # alternating
        for k, fn in makers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(core, fps=30)
            torch.cuda.synchronize()
            t[k].append(core.num_images / (time.perf_counter() - t0))
    for k, v in t.items():
        res[k] = {"frames_per_s_median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    res["ratio_heatmap_over_pose2d"] = res["heatmap"]["frames_per_s_median"] / res["pose2d"]["frames_per_s_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=64, help="images per camera of the generated folder")
    ap.add_argument("--repeats", type=int, default=3, help="timed runs of each video loop")
    ap.add_argument("--folder", default=None, help="a folder of camera images to make the videos from (default: a generated one); 'none' skips the loops")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "launches_per_window": a.launches, "drawing": drawing(dev, a.rounds, a.launches)}
    print(json.dumps(res, indent=1), flush=True)   # the drawing launch's record, before the loops start their encoders
    if a.folder != "none":
        with tempfile.TemporaryDirectory() as tmp:
            res["video_loops"] = loops(a.folder or sample_folder(a.frames, tmp), a.repeats)
    text = json.dumps(res, indent=1)
    if "video_loops" in res:
        print(json.dumps({"video_loops": res["video_loops"]}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
