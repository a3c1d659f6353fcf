"""Seconds per video frame of the Motion-JPEG path's two encoders, on rendered frames of the two video sizes:
2880 x 960 (the pose-2d and heat-map videos) and 600 x 400 (the pose-3d video), 16 frames per batch.

    device   jpeg.JpegFrameEncoder.encode: the kernels, the copy of the sizes and of the scans' bytes, the host putting header and EOI
             round every scan
    pillow   what the writer did before: host.copy_(frame) into a pinned buffer, Image.save(format="JPEG") -- one frame at a time

Both legs run in this process, alternating, after a warm-up batch each: --repeats windows of --frames frames per leg, host clock, the device
idle at both ends of a window.  The device route wins only if its SLOWEST window beats Pillow's FASTEST one: the spread between windows is
the noise, so that is the whole margin.  Needs a GPU; there is no CPU fall-back.

    python tests/perf/jpeg_encode_bench.py [--frames 208] [--repeats 3] [--quality 90] [--out result.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/perf/jpeg_encode_bench.py --device-only --frames 64     # the kernels' shares
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from deepfly3d_amd import jpeg, video  # noqa: E402

BATCH = 16
GOLDEN = os.path.join(ROOT, "tests", "golden")


def rendered_frames(dev):
    """16 frames of each video size, drawn by the renderer from the golden sample: the camera grid with the 2-D pose (the detections shifted a
    little from frame to frame), and the pose-3d layout made from it."""
    H, W, J = 480, 960, 38
    blobs = [open(os.path.join(GOLDEN, "images", f"camera_{c}_img_0.jpg"), "rb").read() for c in video.GRID_CAMERAS]
    luma = jpeg.decode_luma(blobs, W, H, device=dev)
    g2 = np.load(os.path.join(GOLDEN, "golden_2d.npz"))
    g3 = np.load(os.path.join(GOLDEN, "golden_3d.npz"))
    pts = np.stack([g2["points2d"][c, 0] * np.array([float(H), float(W)]) for c in video.GRID_CAMERAS])
    from deepfly3d_amd.procrustes import video_pose

    pose = video.merge_stripes(video_pose(g3["points3d_wo_procrustes"], device=dev))
    r = video.FrameRenderer(H, W, J, dev)
    big = torch.empty((BATCH, 2 * H, 3 * W, 3), dtype=torch.uint8, device=dev)
    sh, sw = video.SMALL_2D
    small = torch.empty((BATCH, 2 * sh + video.PANEL_SIZE, 3 * sw, 3), dtype=torch.uint8, device=dev)
    for k in range(BATCH):
        moved = np.where(pts != 0, pts + 2.0 * k, 0.0)
        r.grid2d(luma, torch.from_numpy(moved).to(dev), out=big[k])
        r.resize(big[k], small[k, : 2 * sh])
        r.panels3d(torch.from_numpy(pose[k % len(pose)]).to(dev).contiguous(), out=small[k, 2 * sh:])
    torch.cuda.synchronize()
    return {"2880x960": big, "600x400": small}


def device_leg(encoder, frames, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(batches):
        n += sum(len(f) for f in encoder.encode(frames))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (batches * BATCH), n / (batches * BATCH)


def pillow_leg(host, frames, batches, quality):
    from PIL import Image

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(batches):
        for k in range(BATCH):
            host.copy_(frames[k])
            buf = io.BytesIO()
            Image.fromarray(host.numpy()).save(buf, format="JPEG", quality=quality)
            n += len(buf.getvalue())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (batches * BATCH), n / (batches * BATCH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=208, help="frames per window (rounded up to whole batches of 16; at least 200 for a figure to quote)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--device-only", action="store_true", help="run the device leg alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("jpeg_encode_bench.py measures the device encoder: it needs a GPU")
    dev = torch.device("cuda:0")
    batches = -(-a.frames // BATCH)
    result = {"batch": BATCH, "frames_per_window": batches * BATCH, "repeats": a.repeats, "quality": a.quality, "device": torch.cuda.get_device_name(0),
              "cpus": len(os.sched_getaffinity(0)), "sizes": {}}
    for name, frames in rendered_frames(dev).items():
        _, h, w, _ = frames.shape
        encoder = jpeg.JpegFrameEncoder(w, h, batch=BATCH, quality=a.quality, device=dev)
        host = torch.empty((h, w, 3), dtype=torch.uint8).pin_memory()
        files = encoder.encode(frames)   # warm-up; and the two routes must agree before either is timed
        if not a.device_only:
            from PIL import Image

            for k in (0, BATCH - 1):
                buf = io.BytesIO()
                Image.fromarray(frames[k].cpu().numpy()).save(buf, format="JPEG", quality=a.quality)
                if buf.getvalue() != files[k]:
                    sys.exit(f"{name}: frame {k} of the device route differs from Pillow's file")
            pillow_leg(host, frames, 1, a.quality)
        dev_s, pil_s, file_bytes = [], [], 0.0
        for _ in range(a.repeats):
            s, file_bytes = device_leg(encoder, frames, batches)
            dev_s.append(s)
            if not a.device_only:
                pil_s.append(pillow_leg(host, frames, batches, a.quality)[0])
        entry = {"device_s_per_frame": dev_s, "file_bytes_per_frame": file_bytes, "device_bytes_to_host_per_frame": encoder.fetch + 16,
                 "pillow_bytes_to_host_per_frame": 3 * w * h, "encoder_retries": encoder.retries}
        if pil_s:
            entry.update(pillow_s_per_frame=pil_s, device_slowest_s=max(dev_s), pillow_fastest_s=min(pil_s), device_wins=max(dev_s) < min(pil_s),
                         ratio_slowest_device_to_fastest_pillow=min(pil_s) / max(dev_s))
        result["sizes"][name] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
