"""f4: the pose videos of `df3d-cli --video-2d / --video-3d` (reference df3d/video.py:21-108, called from df3d/cli.py:308-321).

The reference builds every frame on the host: six `Core.plot_2d` images (matplotlib / cv2 drawing, one image at a time) stacked into a
2 x 3 grid -- cameras 0, 1, 2 over 4, 5, 6 -- and, for the 3-D video, a third row of three matplotlib 3-D plots; cv2.VideoWriter
encodes them.  Here a frame is drawn by ONE kernel launch on the GPU (csrc/render.hip: `df3d_render_pose2d_grid`,
`df3d_render_pose3d_panels`, `df3d_resize_rgb`) from camera frames decoded on the GPU (csrc/jpeg.hip); the host only moves finished RGB
frames to the encoder:

    ffmpeg on PATH   -> raw RGB frames piped into `ffmpeg ... -c:v mpeg4`, the reference's file name  video_pose2d_<folder>.mp4
    no ffmpeg        -> Motion-JPEG in an AVI container written here: same stem, .avi -- this image has neither cv2 nor ffmpeg, and an
                        MP4 muxer is outside the hot path.  The frames are encoded on the device, 16 at a time (csrc/jpeg_encode.hip,
                        DESIGN.md section 27): only the JPEG bytes cross to the host, and they are the bytes Pillow would have written

Same layout, same file naming, same frame rate rule (--output-fps, else the camera videos' rate, else 30) as the reference; the
drawing rule (joint discs over bone segments over the grey image; orthographic 3-D panels) is this build's own and is pinned by
oracle/render.py.  Visualisation only: no result file depends on these pixels.
"""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import torch

from . import _native, logger, ops
from .config import LIMB_COLORS, camera_is_flipped, config, heatmap_planes, limb_of_joint, plane_color, skeleton_bones

DEFAULT_FPS = 30                     # reference video.py:19
GRID_CAMERAS = (0, 1, 2, 4, 5, 6)    # reference video.py:35-36: the front camera (3) is not shown
PANEL_CAMERAS = (4, 5, 6)            # reference video.py:66
PANEL_SIZE = 200                     # img3d_aspect (2, 2) x img3d_dpi 100 (reference video.py:14-15)
SMALL_2D = (100, 200)                # img2d_aspect (2, 1) x 100: (height, width) of one camera image in the 3-D video
JOINT_RADIUS, BONE_WIDTH = 6.0, 3.0  # as Camera.plot_2d draws them (camera_network.py)
PANEL_LINE_WIDTH, PANEL_LIM, PANEL_ELEV = 1.5, 2.0, 30.0   # reference video.py:150-155 (thickness 1.5, lim 2), matplotlib's default elevation


def _tables(num_joints):
    bones = np.asarray([b for b in skeleton_bones() if max(b) < num_joints], dtype=np.int32).reshape(-1, 2)
    rgb = np.asarray([LIMB_COLORS[limb_of_joint(j) % len(LIMB_COLORS)] for j in range(num_joints)], dtype=np.uint8)
    return np.ascontiguousarray(bones), np.ascontiguousarray(rgb)


def panel_azimuths(cameras=PANEL_CAMERAS):
    """matplotlib view_init azimuth per camera (reference plot_util.py:48-51)."""
    return [(-60.0 + 30.0 * c) if c < 3 else (-60.0 + 45.0 * c) for c in cameras]


def merge_stripes(points3d):
    """The stripe joints of the two body sides are the same physical points: both get their mean (reference plot_util.py:62-72)."""
    p = np.array(points3d, dtype=np.float64, copy=True)
    half = p.shape[-2] // 2
    for j in (16, 17, 18):
        if j + half < p.shape[-2]:
            p[..., j, :] = 0.5 * (p[..., j, :] + p[..., j + half, :])
            p[..., j + half, :] = p[..., j, :]
    return p


class FrameRenderer:
    """Device-side drawing of video frames through the C ABI."""

    def __init__(self, height, width, num_joints, device):
        _native.require_gpu()
        self.lib = _native.load()
        self.dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.dev.type == "cuda" and self.dev.index is None:   # "cuda": the current device, by its index (tensors carry one)
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.h, self.w, self.j = height, width, num_joints
        self.bones, self.rgb = _tables(num_joints)
        self._bones_p = self.bones.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self._rgb_p = self.rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _need(self, t, dtype, shape, name):
        """The C ABI reads `t` from its data pointer alone: type, device, shape and layout are settled here."""
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor")
        if t.device != self.dev:
            raise ValueError(f"{name} lives on {t.device}, the renderer on {self.dev}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")

    def _need_rows(self, t, name):
        """[h, w, 3] uint8 with packed pixels; rows may lie apart by a whole number of pixels (a view of a wider or taller image)."""
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3):
            raise ValueError(f"{name} must be a [h, w, 3] {torch.uint8} CUDA tensor")
        if t.device != self.dev:
            raise ValueError(f"{name} lives on {t.device}, the renderer on {self.dev}")
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} must not be empty, got {list(t.shape)}")
        if t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) % 3 != 0 or t.stride(0) < 3 * t.shape[1]:
            raise ValueError(f"{name} must have packed RGB pixels and a row pitch of whole pixels, at least its width; strides {t.stride()}")

    def grid2d(self, luma6, points6, out=None):
        """luma6 [6, H, W] uint8 cuda, points6 [6, J, 2] float64 cuda (row_px, col_px) -> [2 H, 3 W, 3] uint8 cuda."""
        self._need(luma6, torch.uint8, (6, self.h, self.w), "luma6")
        self._need(points6, torch.float64, (6, self.j, 2), "points6")
        if out is None:
            out = torch.empty((2 * self.h, 3 * self.w, 3), dtype=torch.uint8, device=self.dev)
        else:
            self._need(out, torch.uint8, (2 * self.h, 3 * self.w, 3), "out")
        with torch.cuda.device(self.dev):
            _native.check(self.lib.df3d_render_pose2d_grid(luma6.data_ptr(), self.h, self.w, points6.data_ptr(), self.j, self._bones_p, len(self.bones),
                                                           self._rgb_p, JOINT_RADIUS, BONE_WIDTH, out.data_ptr(), self._stream()), "df3d_render_pose2d_grid")
        return out

    def panels3d(self, points3d, out=None, size=PANEL_SIZE):
        """points3d [J, 3] float64 cuda -> [size, 3 size, 3] uint8 cuda."""
        self._need(points3d, torch.float64, (self.j, 3), "points3d")
        if out is None:
            out = torch.empty((size, 3 * size, 3), dtype=torch.uint8, device=self.dev)
        else:
            self._need(out, torch.uint8, (size, 3 * size, 3), "out")
        az = (ctypes.c_double * 3)(*panel_azimuths())
        with torch.cuda.device(self.dev):
            _native.check(self.lib.df3d_render_pose3d_panels(points3d.data_ptr(), self.j, self._bones_p, len(self.bones), self._rgb_p, az, PANEL_ELEV,
                                                             PANEL_LIM, size, PANEL_LINE_WIDTH, out.data_ptr(), self._stream()), "df3d_render_pose3d_panels")
        return out

    def resize(self, img, out):
        """img [h, w, 3] uint8 cuda -> out (a [oh, ow, 3] view of a wider image is fine: row pitch taken from its stride)."""
        self._need_rows(img, "img")
        self._need_rows(out, "out")
        with torch.cuda.device(self.dev):
            _native.check(self.lib.df3d_resize_rgb(img.data_ptr(), img.shape[0], img.shape[1], img.stride(0) // 3, out.data_ptr(), out.shape[0], out.shape[1],
                                                   out.stride(0) // 3, self._stream()), "df3d_resize_rgb")
        return out


    def heatmap_grid(self, luma6, heatmaps6, camera_ordering=None, joints=(), gain=1.0, out=None):
        """luma6 [6, H, W] uint8 cuda and heatmaps6 [6, 19, 64, 128] float32 cuda, the views of GRID_CAMERAS as the network saw them
        -> [2 H, 3 W, 3] uint8 cuda: every camera image with its heat-maps drawn on it (ops.render_heatmap, one launch; DESIGN.md
        section 13).  `joints` restricts the drawing to those ids of the 38-joint layout."""
        pairs = [heatmap_planes(c, joints, camera_ordering) for c in GRID_CAMERAS]
        return ops.render_heatmap(luma6, heatmaps6, [[p for p, _ in pr] for pr in pairs], [[plane_color(j) for _, j in pr] for pr in pairs],
                                  [camera_is_flipped(c, camera_ordering) for c in GRID_CAMERAS], gain=gain, cols=3, out=out)

# ---- encoders ------------------------------------------------------------------------------------------------------------------------
class FfmpegWriter:
    """Raw RGB frames into an ffmpeg child process (mpeg4 in .mp4, like the reference's cv2 'mp4v')."""

    def __init__(self, path, width, height, fps):
        import tempfile

        self.path = path
        self.log = tempfile.TemporaryFile()   # ffmpeg's stderr: a file, so a chatty child can never block on a full pipe
        self.proc = subprocess.Popen(
            ["ffmpeg", "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{width}x{height}", "-r", str(fps), "-i", "-",
             "-c:v", "mpeg4", "-q:v", "3", "-pix_fmt", "yuv420p", path], stdin=subprocess.PIPE, stderr=self.log)

    def _reason(self):
        self.log.seek(0)
        return self.log.read()[-2000:].decode(errors="replace").strip()

    def write(self, frame):
        try:
            self.proc.stdin.write(frame.tobytes())
        except BrokenPipeError:
            self.proc.wait()
            raise RuntimeError(f"ffmpeg exited (code {self.proc.returncode}) while writing {self.path}: {self._reason()}") from None

    def close(self):
        """Always reaps the child; raises for a failed encode only when no other exception is already in flight (a `finally:
        writer.close()` must not mask the error that got us here)."""
        in_flight = sys.exc_info()[1] is not None
        try:
            self.proc.stdin.close()
        except (BrokenPipeError, OSError):
            pass
        code = self.proc.wait()
        reason = self._reason()
        self.log.close()
        if code != 0 and not in_flight:
            raise RuntimeError(f"ffmpeg failed (code {code}) writing {self.path}: {reason}")


class MjpegAviWriter:
    """Motion-JPEG in a RIFF/AVI container: what can be written without ffmpeg.  `write_jpeg` takes a finished JPEG file (the video
    functions encode their frames on the device, jpeg.JpegFrameEncoder); `write` takes an RGB array and has Pillow encode it.  The two give
    the same file.  `device_encode=False` asks the video functions for the Pillow route."""

    def __init__(self, path, width, height, fps, quality=90, device_encode=True):
        self.path, self.w, self.h, self.fps, self.q, self.device_encode = path, width, height, float(fps), quality, bool(device_encode)
        self.f = open(path, "wb")
        self.index = []
        self.limit = (1 << 32) - (1 << 24)   # a plain RIFF/AVI carries 32-bit sizes and idx1 offsets: stop 16 MiB short of 4 GiB
        self.f.write(b"\0" * 224)   # RIFF + hdrl, patched in close()
        self.movi_at = self.f.tell()
        self.f.write(b"LIST\0\0\0\0movi")

    def write(self, frame):
        import io

        from PIL import Image

        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, format="JPEG", quality=self.q)
        self.write_jpeg(buf.getvalue())

    def write_jpeg(self, data):
        """One frame, already encoded: a baseline JPEG file of the writer's size."""
        pad = len(data) & 1
        if self.f.tell() + 8 + len(data) + pad + 16 * (len(self.index) + 1) + 8 > self.limit:
            raise RuntimeError(f"{self.path}: the Motion-JPEG fallback writes a plain RIFF/AVI, which ends at 4 GiB ({len(self.index)} frames written so far); "
                               "install ffmpeg for the .mp4 path, or render fewer frames (-n)")
        self.index.append((self.f.tell() - self.movi_at - 8, len(data)))
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * pad)

    def close(self):
        n = len(self.index)
        movi_end = self.f.tell()
        idx = b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self.index)
        self.f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        end = self.f.tell()
        usec = int(round(1e6 / self.fps))
        biggest = max((s for _, s in self.index), default=0)
        avih = struct.pack("<IIIIIIIIII4I", usec, int(biggest * self.fps), 0, 0x10, n, 0, 1, biggest, self.w, self.h, 0, 0, 0, 0)
        rate, scale = int(round(self.fps * 1000)), 1000
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0) + struct.pack("<hhhh", 0, 0, self.w, self.h)
        strf = struct.pack("<IiiHHIIiiII", 40, self.w, self.h, 1, 24, 0x47504A4D, self.w * self.h * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl_body = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        hdrl = b"LIST" + struct.pack("<I", len(hdrl_body)) + hdrl_body
        junk_len = 224 - 12 - len(hdrl) - 8
        assert junk_len >= 0
        head = b"RIFF" + struct.pack("<I", end - 8) + b"AVI " + hdrl + b"JUNK" + struct.pack("<I", junk_len) + b"\0" * junk_len
        self.f.seek(0)
        self.f.write(head)
        self.f.seek(self.movi_at + 4)
        self.f.write(struct.pack("<I", movi_end - self.movi_at - 8))
        self.f.close()


def open_writer(stem, width, height, fps, quality=90, device_encode=True):
    """The encoder for `<stem>.mp4` (ffmpeg) or, without ffmpeg, `<stem>.avi` (Motion-JPEG at JPEG quality `quality`, its frames encoded
    on the device unless `device_encode=False`).  Returns (writer, path)."""
    if shutil.which("ffmpeg"):
        path = stem + ".mp4"
        return FfmpegWriter(path, width, height, fps), path
    path = stem + ".avi"
    logger.warning(f"ffmpeg is not on PATH: writing Motion-JPEG to {path} instead of the reference's .mp4")
    return MjpegAviWriter(path, width, height, fps, quality=quality, device_encode=device_encode), path


ENCODE_BATCH = 16   # device frames per JPEG-encoder call


def _write_frames(writer, frames, width, height, device, progress=None):
    """Every (img_id, [height, width, 3] uint8 cuda) of `frames` into `writer`.  The Motion-JPEG writer gets JPEG files encoded on the device,
    ENCODE_BATCH frames per call; any other writer (and `device_encode=False`) gets the RGB frames through one pinned host buffer."""
    if isinstance(writer, MjpegAviWriter) and writer.device_encode:
        from . import jpeg

        dev = torch.device(device)
        encoder = jpeg.JpegFrameEncoder(width, height, batch=ENCODE_BATCH, quality=writer.q, device=dev)
        stage = torch.empty((ENCODE_BATCH, height, width, 3), dtype=torch.uint8, device=dev)
        held = 0

        def flush():
            for data in encoder.encode(stage[:held]):
                writer.write_jpeg(data)
                if progress is not None:
                    progress()

        for _, frame in frames:
            stage[held].copy_(frame)    # (the renderers reuse their output buffers)
            held += 1
            if held == ENCODE_BATCH:
                flush()
                held = 0
        if held:
            flush()
        return
    host = torch.empty((height, width, 3), dtype=torch.uint8).pin_memory()
    for _, frame in frames:
        host.copy_(frame)
        writer.write(host.numpy())
        if progress is not None:
            progress()


def read_mjpeg_avi(path):
    """[frame ndarray, ...] of a file MjpegAviWriter wrote (tests, and a quick look without a player)."""
    import io

    from PIL import Image

    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    at = data.index(b"movi") + 4
    idx_at = data.rindex(b"idx1")
    frames = []
    while at < idx_at and data[at:at + 4] == b"00dc":
        size = struct.unpack_from("<I", data, at + 4)[0]
        frames.append(np.asarray(Image.open(io.BytesIO(data[at + 8:at + 8 + size])).convert("RGB")))
        at += 8 + size + (size & 1)
    return frames


# ---- the two videos ------------------------------------------------------------------------------------------------------------------
def _frame_files(core, img_id):
    out = []
    for cam in GRID_CAMERAS:
        path = core._image_path.format(cam_id=cam, img_id=img_id)
        if not os.path.exists(path):
            path = core._image_path.format(cam_id=cam, img_id=f"{img_id:06d}")
        out.append(path)
    return out


def _grid_frames(core, renderer, batch=16, smooth=False):
    """Yield (img_id, [2 H, 3 W, 3] uint8 cuda) for every image of the recording: files -> device JPEG decode -> one drawing launch.
    `smooth`: draw the temporally smoothed detections (Core.smooth_points2d) instead of the detections."""
    from . import jpeg

    W, H = core.image_shape
    per_cam = core.smooth_points2d if smooth else (lambda c: core.camNet.cam_list[c].points2d)
    pts = np.stack([per_cam(c)[: core.num_images] for c in GRID_CAMERAS], axis=1)   # (T, 6, J, 2) pixels (row, col)
    pts_dev = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(renderer.dev)
    for t0 in range(0, core.num_images, batch):
        ids = range(t0, min(t0 + batch, core.num_images))
        blobs = [open(p, "rb").read() for i in ids for p in _frame_files(core, i)]
        luma = jpeg.decode_luma(blobs, W, H, device=renderer.dev).reshape(len(ids), 6, H, W)
        for k, i in enumerate(ids):
            yield i, renderer.grid2d(luma[k], pts_dev[i])


def _video_stem(core, kind):
    return os.path.join(core.output_folder, f"video_{kind}_" + core.input_folder.replace("/", "_"))


def make_pose2d_video(core, fps=None, progress=None, smooth=False, quality=90, device_encode=True):
    """video_pose2d_<folder>: per image the 2 x 3 camera grid with the 2-D pose drawn on it (reference video.py:21-49).  Returns the path.
    `smooth=True` draws the temporally smoothed detections; the default draws the detections themselves.
    `quality` (1 .. 100) and `device_encode` act on the Motion-JPEG path only (open_writer)."""
    fps = fps or DEFAULT_FPS
    W, H = core.image_shape
    renderer = FrameRenderer(H, W, config["num_joints"], core.device)
    writer, path = open_writer(_video_stem(core, "pose2d"), 3 * W, 2 * H, fps, quality=quality, device_encode=device_encode)
    try:
        # (progress: multi-rank, rank 0's heartbeat to the waiting peers, distributed.primary_section)
        _write_frames(writer, _grid_frames(core, renderer, smooth=smooth), 3 * W, 2 * H, renderer.dev, progress)
    finally:
        writer.close()
    logger.info(f"Video created at {path}\n")
    return path


def make_pose3d_video(core, fps=None, progress=None, quality=90, device_encode=True):
    """video_pose3d_<folder>: two rows of the six camera images with their 2-D pose (200 x 100 each) over a row of three 3-D views of
    the pose `Core.get_points3d` returns (reference video.py:52-82).  Returns the path.  `quality`, `device_encode`: as in make_pose2d_video."""
    fps = fps or DEFAULT_FPS
    W, H = core.image_shape
    renderer = FrameRenderer(H, W, config["num_joints"], core.device)
    pose = torch.from_numpy(merge_stripes(core.get_points3d())).to(renderer.dev)   # (T, J, 3)
    sh, sw = SMALL_2D
    fw, fh = 3 * sw, 2 * sh + PANEL_SIZE
    frame = torch.empty((fh, fw, 3), dtype=torch.uint8, device=renderer.dev)
    writer, path = open_writer(_video_stem(core, "pose3d"), fw, fh, fps, quality=quality, device_encode=device_encode)

    def frames():
        for i, grid in _grid_frames(core, renderer):
            renderer.resize(grid, frame[: 2 * sh])
            renderer.panels3d(pose[i].contiguous(), out=frame[2 * sh:])
            yield i, frame

    try:
        _write_frames(writer, frames(), fw, fh, renderer.dev, progress)
    finally:
        writer.close()
    logger.info(f"Video created at {path}\n")
    return path


def _heatmap_frames(core, renderer, batch=16, joints=()):
    """Yield (img_id, [2 H, 3 W, 3] uint8 cuda) for every image: files -> device JPEG decode -> the hourglass on the batch's six views per
    image -> one drawing launch per frame.  One batch of heat-maps (4.3 MB per frame) lives on the device at a time; none reaches the host."""
    from . import jpeg
    from .inference import PREPROCESS, get_engine

    W, H = core.image_shape
    engine = get_engine(dtype=core.dtype, device=renderer.dev)
    flip6 = torch.tensor([1 if camera_is_flipped(c, core.camera_ordering) else 0 for c in GRID_CAMERAS], dtype=torch.uint8, device=renderer.dev)

    def forward(e, luma, flip):
        return e.forward_u8(luma, flip, PREPROCESS["mean"], PREPROCESS["std"], resize=PREPROCESS["resize"])

    for t0 in range(0, core.num_images, batch):
        ids = range(t0, min(t0 + batch, core.num_images))
        blobs = [open(p, "rb").read() for i in ids for p in _frame_files(core, i)]
        luma = jpeg.decode_luma(blobs, W, H, device=renderer.dev)   # [6 n, H, W], image-major
        flip = flip6.repeat(len(ids))
        if t0 == 0 and engine.dtype != "f32":   # a reduced-precision engine proves itself on the first image's views (HourglassEngine.canary)
            engine.canary(get_engine(dtype="f32", device=renderer.dev), lambda e: forward(e, luma[:6], flip[:6]), what=f"the first views of {core.input_folder}")
        hm = forward(engine, luma, flip)
        luma, hm = luma.reshape(len(ids), 6, H, W), hm.reshape(len(ids), 6, *hm.shape[1:])
        for k, i in enumerate(ids):
            yield i, renderer.heatmap_grid(luma[k], hm[k], core.camera_ordering, joints)


def make_heatmap_video(core, fps=None, progress=None, joints=(), quality=90, device_encode=True):
    """video_heatmap_<folder>: per image the 2 x 3 camera grid of the pose-2d video with the network's heat-maps drawn on the images
    instead of the pose.  Needs the images and the weights only, not a pose.  `joints` restricts the drawing to
    those ids of the 38-joint layout.  Returns the path.  `quality`, `device_encode`: as in make_pose2d_video."""
    if not core.has_heatmap:
        raise FileNotFoundError(f"the heat-map video is computed from the images, and {core.input_folder} holds none (deleted with --delete-images?)")
    fps = fps or DEFAULT_FPS
    W, H = core.image_shape
    renderer = FrameRenderer(H, W, config["num_joints"], core.device)
    writer, path = open_writer(_video_stem(core, "heatmap"), 3 * W, 2 * H, fps, quality=quality, device_encode=device_encode)
    try:
        _write_frames(writer, _heatmap_frames(core, renderer, joints=joints), 3 * W, 2 * H, renderer.dev, progress)
    finally:
        writer.close()
    logger.info(f"Video created at {path}\n")
    return path
