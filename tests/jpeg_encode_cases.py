"""The frames the JPEG-encoder tests share (tests/test_jpeg_encode_host.py, tests/test_gpu_jpeg_encode.py): (H, W, content, quality)."""
import io

import numpy as np

CASES = [(1, 1, "noise", 90), (9, 7, "noise", 90), (16, 16, "smooth", 90), (37, 50, "smooth", 90), (40, 48, "noise", 90), (33, 17, "noise", 75),
         (24, 40, "noise", 100), (24, 40, "saturated", 100), (100, 60, "smooth", 50), (44, 22, "noise", 85), (18, 34, "noise", 30), (35, 21, "noise", 10),
         (24, 24, "noise", 1), (32, 48, "constant", 90), (50, 34, "saturated", 25), (17, 33, "noise", 49), (70, 130, "noise", 90)]
QUALITIES = (1, 25, 49, 50, 75, 90, 95, 100)


def case_id(case):
    return "{}x{}-{}-q{}".format(*case)


def frame(h, w, content, seed=0):
    """[h, w, 3] uint8."""
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    if content == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if content == "saturated":      # every sample 0 or 255: the largest coefficients the transform can give
        return (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    if content == "constant":
        return np.broadcast_to(np.array([255, 0, 128], np.uint8), (h, w, 3)).copy()
    if content == "smooth":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        ph = rng.uniform(0, 6.28, size=3)
        img = np.stack([127.5 + 120 * np.sin(0.07 * xx + 0.05 * yy + ph[0]), 127.5 + 120 * np.cos(0.04 * xx - 0.09 * yy + ph[1]),
                        127.5 + 100 * np.sin(0.11 * yy + ph[2]) * np.cos(0.03 * xx)], axis=-1)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)
    raise ValueError(content)


def pillow_file(rgb, quality):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()
