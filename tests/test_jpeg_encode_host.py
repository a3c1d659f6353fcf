"""CPU tests of the JPEG encoder's host side: the numpy oracle against Pillow (byte for byte), the quantisation
tables and the header the package builds, the argument checks of the two C-ABI entries, and MjpegAviWriter.write_jpeg."""
import ctypes
import io
import struct

import numpy as np
import pytest

import jpeg_encode_oracle as oracle
from jpeg_encode_cases import CASES, QUALITIES, case_id, frame, pillow_file


def _pillow_tables(blob):
    """The DQT tables of a JPEG file, natural order: {id: [64]}."""
    out, at = {}, 2
    while blob[at + 1] != 0xDA:
        length = struct.unpack_from(">H", blob, at + 2)[0]
        if blob[at + 1] == 0xDB:
            body = blob[at + 4:at + 2 + length]
            nat = np.zeros(64, np.uint8)
            nat[oracle.ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
            out[body[0]] = nat
        at += 2 + length
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_file_equals_pillow(case):
    h, w, content, quality = case
    rgb = frame(h, w, content)
    assert oracle.file(rgb, quality) == pillow_file(rgb, quality)


def test_oracle_stages_are_consistent():
    rgb = frame(37, 50, "noise")
    coef = oracle.coefficients(rgb, 90)
    assert coef.shape == (6 * 4 * 3, 64) and coef.dtype == np.int16
    bits = oracle.block_bits(coef)
    raw = oracle.unstuffed(coef)
    assert len(raw) == (bits.sum() + 7) // 8 and bits.min() >= 4 and bits.max() <= 1658
    assert oracle.scan(coef).replace(b"\xff\x00", b"\xff") == raw
    y, cb, cr = oracle.planes(rgb)
    assert y.shape == (40, 56) and cb.shape == cr.shape == (24, 32)
    # a dummy luma column: W = 50 has 7 block columns in 4 MCUs; the eighth block repeats the DC of the seventh and has no AC
    assert np.array_equal(coef[3 * 6 + 1, 1:], np.zeros(63)) and coef[3 * 6 + 1, 0] == coef[3 * 6 + 0, 0]


@pytest.mark.parametrize("quality", QUALITIES)
def test_quality_tables_and_header_equal_pillows(quality):
    from deepfly3d_amd import jpeg

    rgb = frame(20, 30, "noise")
    blob = pillow_file(rgb, quality)
    luma, chroma = jpeg.quality_tables(quality)
    assert luma.dtype == chroma.dtype == np.uint8 and luma.shape == chroma.shape == (64,)
    tabs = _pillow_tables(blob)
    assert np.array_equal(luma, tabs[0]) and np.array_equal(chroma, tabs[1])
    head = jpeg.jfif_header(30, 20, quality)
    assert blob[:len(head)] == head and head == oracle.header(30, 20, quality)
    assert blob[len(head) - 14:len(head) - 10] == b"\xff\xda\x00\x0c"     # the header ends with the SOS segment: the scan follows


def test_quality_and_size_checks():
    from deepfly3d_amd import jpeg

    for bad in (0, 101, 50.5):
        with pytest.raises(ValueError):
            jpeg.quality_tables(bad)
    with pytest.raises(ValueError):
        jpeg.jfif_header(0, 10, 90)
    with pytest.raises(ValueError):
        jpeg.jfif_header(10, 65536, 90)


def test_encode_entries_check_their_arguments(native_lib):
    """Argument errors come before any device work, so this runs without a GPU."""
    lib = native_lib
    p = ctypes.c_void_p(4096)
    ok = (ctypes.c_ubyte * 64)(*([16] * 64))
    zero = (ctypes.c_ubyte * 64)(*([16] * 63 + [0]))
    need = lib.df3d_jpeg_encode_work_bytes(16, 2880, 960)
    blocks = 6 * 180 * 60
    assert need >= 16 * blocks * (128 + 4 + 208)      # coefficients, bits, the unstuffed stream's worst case
    assert lib.df3d_jpeg_encode_work_bytes(0, 8, 8) >= 0 and lib.df3d_jpeg_encode_work_bytes(1, 1, 1) > 0
    assert lib.df3d_jpeg_encode_work_bytes(-1, 8, 8) == 0 and lib.df3d_jpeg_encode_work_bytes(1, 0, 8) == 0
    assert lib.df3d_jpeg_encode_work_bytes(1, 8, 65536) == 0

    def call(rgb=p, n=1, h=8, w=8, ql=ok, qc=ok, out=p, cap=1024, sizes=p, status=p, work=p, work_bytes=1 << 40):
        return lib.df3d_jpeg_encode_rgb(rgb, n, h, w, ql, qc, out, cap, sizes, status, work, work_bytes, None, None, None)

    for kwargs, needle in ((dict(n=-1), b"n must not be negative"), (dict(w=0), b"1 .. 65535"), (dict(h=65536), b"1 .. 65535"), (dict(rgb=None), b"null pointer"),
                           (dict(out=None), b"null pointer"), (dict(sizes=None), b"null pointer"), (dict(status=None), b"null pointer"),
                           (dict(work=None), b"null pointer"), (dict(ql=None), b"null pointer"), (dict(qc=zero), b"1 .. 255"),
                           (dict(work_bytes=16), b"work buffer too small"), (dict(w=65535, h=65535), b"32-bit")):
        assert call(**kwargs) == -1 and needle in lib.df3d_last_error(), kwargs
    assert lib.df3d_last_error().startswith(b"df3d_jpeg_encode_rgb: ")
    assert lib.df3d_jpeg_encode_rgb(None, 0, 8, 8, None, None, None, 0, None, None, None, 0, None, None, None) == 0   # an empty batch


def test_write_jpeg_gives_the_file_write_gives(tmp_path):
    from deepfly3d_amd import video

    frames = [frame(34, 50, kind, seed=k) for k, kind in enumerate(("noise", "smooth", "saturated"))]
    a, b = str(tmp_path / "a.avi"), str(tmp_path / "b.avi")
    wa = video.MjpegAviWriter(a, 50, 34, 25, quality=80)
    wb = video.MjpegAviWriter(b, 50, 34, 25, quality=80, device_encode=False)
    assert wa.device_encode and not wb.device_encode
    for f in frames:
        wa.write_jpeg(pillow_file(f, 80))
        wb.write(f)
    wa.close()
    wb.close()
    assert open(a, "rb").read() == open(b, "rb").read()
    back = video.read_mjpeg_avi(a)
    assert len(back) == 3 and back[0].shape == (34, 50, 3)


def test_video_functions_take_quality_and_the_cli_flag_is_checked():
    import inspect

    from deepfly3d_amd import cli, video

    for fn in (video.make_pose2d_video, video.make_pose3d_video, video.make_heatmap_video):
        assert inspect.signature(fn).parameters["quality"].default == 90
    assert inspect.signature(video.open_writer).parameters["quality"].default == 90
    assert cli.parse_cli_args(["/tmp/x"]).video_quality == 90 and cli.parse_cli_args(["/tmp/x", "--video-quality", "50"]).video_quality == 50
    for bad in ("0", "101"):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(["/tmp/x", "--video-quality", bad])
