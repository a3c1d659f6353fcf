"""-m gpu: the device JPEG encoder (csrc/jpeg_encode.hip, deepfly3d_amd/jpeg.py).

Every comparison is an equality: the stages against tests/jpeg_encode_oracle.py, whole files against Pillow, the videos written through the
device encoder against those written through Pillow."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_encode_oracle as oracle
from jpeg_encode_cases import CASES, case_id, frame, pillow_file

pytestmark = pytest.mark.gpu


def _encode(frames, quality, capacity, cuda, guard=0, stages=False):
    """The C ABI on [n, H, W, 3] uint8 numpy -> (the slots [n, capacity] followed by `guard` bytes, flat; sizes; status; coef; bits).  Slots and
    guard are filled with 0xA5 before the call."""
    from deepfly3d_amd import _native, jpeg

    lib = _native.load()
    n, h, w, _ = frames.shape
    dev = torch.from_numpy(frames).to(cuda)
    blocks = jpeg.blocks_per_frame(w, h)
    work = torch.empty((lib.df3d_jpeg_encode_work_bytes(n, w, h),), dtype=torch.uint8, device=cuda)
    out = torch.full((n * capacity + guard,), 0xA5, dtype=torch.uint8, device=cuda)
    sizes = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    status = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    coef = torch.full((n, blocks, 64), 0x5A5A, dtype=torch.int16, device=cuda) if stages else None
    bits = torch.full((n, blocks), -1, dtype=torch.int32, device=cuda) if stages else None
    jpeg.encode_scans(dev, jpeg.quality_tables(quality), out[:n * capacity].view(n, capacity), sizes, status, work, coef=coef, bits=bits)
    torch.cuda.synchronize()
    return out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy(), None if coef is None else coef.cpu().numpy(), None if bits is None else bits.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stages_equal_the_oracle(native_lib, cuda, case):
    """Coefficients (dummy blocks included), bits per block and the scan, exactly.  The capacity has a guard behind it."""
    h, w, content, quality = case
    rgb = frame(h, w, content)
    want_coef = oracle.coefficients(rgb, quality)
    want_scan = oracle.scan(want_coef)
    out, sizes, status, coef, bits = _encode(rgb[None], quality, len(want_scan), cuda, guard=64, stages=True)
    assert np.array_equal(coef[0], want_coef)
    assert np.array_equal(bits[0], oracle.block_bits(want_coef))
    assert status[0] == 0 and sizes[0] == len(want_scan)
    assert out[:len(want_scan)].tobytes() == want_scan      # a slot of exactly the scan's size
    assert (out[len(want_scan):] == 0xA5).all() and out.size == len(want_scan) + 64


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_files_equal_pillows(native_lib, cuda, case):
    from deepfly3d_amd import jpeg

    h, w, content, quality = case
    rgb = frame(h, w, content)
    files = jpeg.encode_rgb(torch.from_numpy(rgb).to(cuda), quality=quality)
    assert len(files) == 1 and files[0] == pillow_file(rgb, quality)


@pytest.mark.parametrize("shape", [(400, 600), (960, 2880)], ids=["400x600", "960x2880"])
def test_video_sized_frames_equal_pillows(native_lib, cuda, shape):
    """The two frame sizes the videos use: 600 x 400 (75 luma block columns in 38 MCUs: a dummy column) and 2880 x 960.  Smooth content with
    noise on a band, like a camera image with a drawing on it."""
    from deepfly3d_amd import jpeg

    h, w = shape
    rgb = frame(h, w, "smooth")
    rgb[h // 3:h // 3 + 40, :, :] = frame(40, w, "noise")
    files = jpeg.encode_rgb(torch.from_numpy(rgb).to(cuda), quality=90)
    assert files[0] == pillow_file(rgb, 90)


def test_a_batch_of_different_frames(native_lib, cuda):
    """Five frames of different content in one call (37 x 50: odd sizes, so the second frame's base address is not dword aligned): per-frame
    sizes and offsets, and the DC predictor starting at 0 in every frame."""
    from deepfly3d_amd import jpeg

    kinds = ("noise", "smooth", "constant", "saturated", "noise")
    rgb = np.stack([frame(37, 50, kind, seed=k) for k, kind in enumerate(kinds)])
    want = [pillow_file(f, 85) for f in rgb]
    assert len({len(x) for x in want}) == 5
    assert jpeg.encode_rgb(torch.from_numpy(rgb).to(cuda), quality=85) == want
    enc = jpeg.JpegFrameEncoder(50, 37, batch=8, quality=85, device=cuda)
    assert enc.encode(torch.from_numpy(rgb[:3]).to(cuda)) == want[:3] and enc.encode(torch.from_numpy(rgb[3:]).to(cuda)) == want[3:]   # buffers reused
    assert enc.encode(torch.from_numpy(rgb[:0]).to(cuda)) == [] and enc.retries == 0
    assert enc.fetch == 4096 < enc.capacity      # 1.25 x the largest scan seen, at least 4 KiB: less than the slot


def test_capacity_is_respected_and_the_encoder_retries(native_lib, cuda):
    """Slots of 64 bytes for noise at quality 100 (scans of some 2 KB).  The constant frame between the noise frames has a scan of a few bytes:
    the rest of its slot is the guard behind the first frame's, the bytes after the last slot the guard behind the last frame's."""
    from deepfly3d_amd import jpeg

    rgb = np.stack([frame(40, 48, kind, seed=k) for k, kind in enumerate(("noise", "constant", "noise"))])
    want = [oracle.scan(oracle.coefficients(f, 100)) for f in rgb]
    out, sizes, status, _, _ = _encode(rgb, 100, 64, cuda, guard=4096)
    assert list(sizes) == [len(x) for x in want] and sizes[0] > 1000 and sizes[2] > 1000 and sizes[1] < 64
    assert list(status) == [1, 0, 1]
    slots = out[:3 * 64].reshape(3, 64)
    assert slots[0].tobytes() == want[0][:64] and slots[2].tobytes() == want[2][:64]
    assert slots[1, :sizes[1]].tobytes() == want[1] and (slots[1, sizes[1]:] == 0xA5).all() and (out[3 * 64:] == 0xA5).all()
    enc = jpeg.JpegFrameEncoder(48, 40, batch=3, quality=100, device=cuda, capacity=64)
    files = enc.encode(torch.from_numpy(rgb).to(cuda))
    assert files == [pillow_file(f, 100) for f in rgb] and enc.retries == 1 and enc.capacity >= max(sizes)      # never truncated
    assert enc.encode(torch.from_numpy(rgb[1:]).to(cuda)) == files[1:] and enc.retries == 1


def test_round_trip_through_the_device_decoder(native_lib, cuda):
    from PIL import Image

    from deepfly3d_amd import jpeg

    rgb = np.stack([frame(100, 60, "smooth", seed=1), frame(100, 60, "noise", seed=2)])
    files = jpeg.encode_rgb(torch.from_numpy(rgb).to(cuda), quality=90)
    luma = jpeg.decode_luma(files, 60, 100, device=cuda).cpu().numpy()
    for k, f in enumerate(rgb):
        img = Image.open(io.BytesIO(pillow_file(f, 90)))
        img.draft("L", img.size)       # libjpeg's own grayscale output: the luma plane
        assert np.array_equal(luma[k], np.asarray(img.convert("L")))


def test_two_runs_are_bit_equal(native_lib, cuda):
    rgb = np.stack([frame(70, 130, "noise", seed=k) for k in range(4)])
    a = _encode(rgb, 95, 32768, cuda, stages=True)
    b = _encode(rgb, 95, 32768, cuda, stages=True)
    assert (a[2] == 0).all()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)      # (bytes past a scan's end keep the fill value in both)


def test_videos_equal_the_pillow_routes(native_lib, cuda, tmp_path, golden_dir, monkeypatch):
    """The golden recording's pose-2d and pose-3d videos (18 frames: one full encoder batch and a short one): the .avi written through the
    device encoder is the file the Pillow route writes; quality 50 gives a smaller one whose frames decode."""
    from test_gpu_reproj import ORDER, _folder, _resumed_core

    from deepfly3d_amd import cli, video
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    monkeypatch.setattr(video.shutil, "which", lambda name: None)      # the Motion-JPEG path, also where ffmpeg is installed
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    p2 = np.concatenate([g3["points2d"], g3["points2d"][:, :3]], axis=1)   # 18 frames
    core = _resumed_core(_folder(tmp_path, golden_dir, 18), golden_dir, p2)
    core.camNet.triangulate()
    for make in (video.make_pose2d_video, video.make_pose3d_video):
        path = make(core, fps=10)
        assert path.endswith(".avi")
        device_file = open(path, "rb").read()
        make(core, fps=10, device_encode=False)
        assert open(path, "rb").read() == device_file
    path = video.make_pose2d_video(core, fps=10)
    at_90 = open(path, "rb").read()
    folder = core.input_folder
    del core
    args = [folder, "--skip-pose-estimation", "--video-2d", "--output-fps", "10", "--order", *[str(c) for c in ORDER]]
    assert cli.main(args) == 0 and open(path, "rb").read() == at_90        # the flag's default is the quality the videos had
    assert cli.main(args + ["--video-quality", "50"]) == 0
    assert os.path.getsize(path) < len(at_90)
    frames = video.read_mjpeg_avi(path)
    assert len(frames) == 18 and frames[0].shape == (960, 2880, 3)
    config.pop("image_shape", None)
