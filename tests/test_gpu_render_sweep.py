"""-m gpu: the three older drawing kernels of csrc/render.hip -- render_pose2d_kernel, render_pose3d_kernel, resize_rgb_kernel -- swept
over sizes, table limits and edge inputs against oracle/render.py, bit for bit (render.hip is built without multiply-add fusion for
exactly this; tests/test_render_oracle_host.py checks the oracle itself against a pixel-by-pixel statement of the rule).

tests/test_gpu_video.py compares the product's frame (480 x 960, 38 joints, the product skeleton, a 200-pixel panel, one resize) through
FrameRenderer, which fixes the bone table, the colours and the view angles.  Here the C ABI is called directly, so that the tables are
the test's own: 1, 19, 38 and 64 joints (MAXJ), 0, a few and 96 bones (MAXB), pairwise distinct random colours -- which make `later
entries win`, `joints over bones` and `a bone takes its FIRST joint's colour` visible in the pixels --, widths on both sides of the
256-pixel x tile, radius and line width 0, joints that are unseen, coincident, off the image or not finite, pitched views, and the
argument checks.  Every output sits inside a larger buffer filled with 0xA5, with 4096 guard bytes on both sides: every byte outside
the frame must stay, every pixel inside must equal the oracle, and the inputs must be unchanged.

Frames are tiny (the largest is 10 x 1539): a case is a handful of launches and numpy masks."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import render as orr

pytestmark = pytest.mark.gpu

GUARD, POISON = 4096, 0xA5
EINVAL = -1   # DF3D_EINVAL of include/df3d_hip.h


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def _stream(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _up(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))


def _guarded(cuda, nbytes):
    """(buffer, pointer to its payload): GUARD poisoned bytes, nbytes poisoned bytes of payload, GUARD poisoned bytes."""
    buf = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=cuda)
    return buf, buf.data_ptr() + GUARD


def _payload(buf, shape):
    """The payload of a _guarded buffer as an array, after checking that both guards are intact."""
    host = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert host.size == 2 * GUARD + n
    assert (host[:GUARD] == POISON).all(), "bytes before the frame were written"
    assert (host[GUARD + n:] == POISON).all(), "bytes behind the frame were written"
    return host[GUARD:GUARD + n].reshape(shape)


def _same_bytes(dev_tensor, host_array):
    return dev_tensor.cpu().numpy().tobytes() == host_array.tobytes()   # bytes: a NaN must stay the NaN it was


def distinct_colours(rng, n):
    """n pairwise distinct RGB triples, none of them grey and none the poison (either could pass for an undrawn pixel)."""
    seen, out = {(POISON,) * 3}, []
    while len(out) < n:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if c not in seen and not (c[0] == c[1] == c[2]):
            seen.add(c)
            out.append(c)
    return np.ascontiguousarray(out, dtype=np.uint8)


def _bones(pairs):
    return np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))


def run_pose2d(lib, cuda, luma, pts, bones, rgb, radius, line_width):
    """df3d_render_pose2d_grid into a guarded buffer -> [2 H, 3 W, 3]; guards and inputs checked."""
    _, H, W = luma.shape
    J = pts.shape[1]
    luma_d, pts_d = torch.from_numpy(luma).to(cuda), torch.from_numpy(pts).to(cuda)
    buf, out_p = _guarded(cuda, 2 * H * 3 * W * 3)
    with torch.cuda.device(cuda):
        rc = lib.df3d_render_pose2d_grid(luma_d.data_ptr(), H, W, pts_d.data_ptr(), J, _ip(bones) if len(bones) else None, len(bones), _up(rgb),
                                         float(radius), float(line_width), out_p, _stream(cuda))
    assert rc == 0, lib.df3d_last_error()
    got = _payload(buf, (2 * H, 3 * W, 3))
    assert _same_bytes(luma_d, luma) and _same_bytes(pts_d, pts), "an input was written"
    return got


def run_pose3d(lib, cuda, p3, bones, rgb, az3, elev, lim, size, line_width):
    p3_d = torch.from_numpy(p3).to(cuda)
    buf, out_p = _guarded(cuda, size * 3 * size * 3)
    with torch.cuda.device(cuda):
        rc = lib.df3d_render_pose3d_panels(p3_d.data_ptr(), p3.shape[0], _ip(bones) if len(bones) else None, len(bones), _up(rgb),
                                           (ctypes.c_double * 3)(*az3), float(elev), float(lim), size, float(line_width), out_p, _stream(cuda))
    assert rc == 0, lib.df3d_last_error()
    got = _payload(buf, (size, 3 * size, 3))
    assert _same_bytes(p3_d, p3), "the input was written"
    return got


def run_resize(lib, cuda, img, oh, ow, pitched):
    """df3d_resize_rgb of img [ih, iw, 3]; pitched: the input is a view of an image 5 pixels wider (other content beside it) and the output a
    view of an image 3 pixels wider, whose other pixels must keep the poison."""
    ih, iw = img.shape[:2]
    in_pitch, out_pitch = (iw + 5, ow + 3) if pitched else (iw, ow)
    wide = np.random.default_rng(99).integers(0, 256, (ih, in_pitch, 3), dtype=np.uint8)
    wide[:, :iw] = img
    wide_d = torch.from_numpy(wide).to(cuda)
    buf, out_p = _guarded(cuda, oh * out_pitch * 3)
    with torch.cuda.device(cuda):
        rc = lib.df3d_resize_rgb(wide_d.data_ptr(), ih, iw, in_pitch, out_p, oh, ow, out_pitch, _stream(cuda))
    assert rc == 0, lib.df3d_last_error()
    full = _payload(buf, (oh, out_pitch, 3))
    assert (full[:, ow:] == POISON).all(), "bytes in the pitch gap were written"
    assert _same_bytes(wide_d, wide), "the input was written"
    return full[:, :ow]


# ---- pose2d ----------------------------------------------------------------------------------------------------------------------------
SIZES_2D = [(1, 1), (3, 255), (2, 256), (2, 257), (5, 513), (7, 300)]
# the bones every table of 19 or more joints starts with: (0, 1) and (2, 1) meet in joint 1; (5, 6) is a point in slot 1; (7, 9), (8, 9) hang on
# joints that slot 2 does not see; 10 .. 13 are not finite in slots 3 and 4; (4, 4) is a disc; (3, 4) runs corner to corner
FEW = [(0, 1), (2, 1), (5, 6), (7, 9), (8, 9), (10, 9), (11, 12), (13, 1), (4, 4), (3, 4)]
TABLES_2D = [(1, 0), (1, 3), (1, 96), (19, 0), (19, len(FEW)), (19, 96), (64, 0), (64, 96)]
RADII, WIDTHS = (0.0, 0.5, 3.0, 1e9), (0.0, 1.0, 2.5)


def points_2d(rng, H, W, J):
    """[6, J, 2] (row, col): quarter-pixel positions in [-10, H + 10] x [-10, W + 10], none exactly 0, with the designed joints."""
    pts = np.stack([rng.integers(-40, 4 * (H + 10) + 1, (6, J)), rng.integers(-40, 4 * (W + 10) + 1, (6, J))], axis=-1) / 4.0
    pts[pts == 0.0] = 0.25
    if J == 1:
        pts[1, 0] = (0.25, 0.25)                        # next to pixel (0, 0)
        pts[2, 0, 0] = 0.0                              # unseen by its row
        pts[3, 0, 1] = np.nan
        pts[5, 0, 1] = 0.0                              # unseen by its column
        return pts
    pts[:, 1] = (0.25, 0.25)                            # within 0.36 of pixel (0, 0): under both bones that meet here and under its own disc
    if H >= 2 and W >= 2:
        pts[:, 3] = (1.0, 1.0)                          # ON a pixel (a joint on row or column 0 would be unseen)
        pts[:, 4] = (float(H - 1), float(W - 1))        # on the last pixel of the last x tile
    pts[1, 6] = pts[1, 5]                               # coincident: a degenerate bone
    pts[2, 7, 0], pts[2, 8, 1] = 0.0, 0.0               # unseen by the row alone, by the column alone
    pts[3, 10, 0], pts[3, 11, 1] = np.nan, np.inf
    pts[4, 12, 0], pts[4, 13] = -np.inf, (1e300, 1e300)
    return pts


def table_2d(rng, J, nb):
    if J == 1:
        return _bones([(0, 0)] * nb)
    return _bones((FEW + [tuple(int(v) for v in rng.integers(0, J, 2)) for _ in range(96)])[:nb])


def _draws(p):
    """A joint that is seen AND can be near a pixel: the last of them owns every pixel at radius 1e9."""
    return p[0] != 0.0 and p[1] != 0.0 and abs(p[0]) < 1e8 and abs(p[1]) < 1e8   # (a NaN fails the last two)


@pytest.mark.parametrize("J,nb", TABLES_2D, ids=lambda v: str(v))
@pytest.mark.parametrize("H,W", SIZES_2D, ids=lambda v: str(v))
def test_pose2d_grid_over_sizes_tables_and_edges(native_lib, cuda, H, W, J, nb):
    rng = np.random.default_rng(1000 * H + W + 7 * J + nb)
    luma = rng.integers(0, 256, (6, H, W), dtype=np.uint8)
    pts, bones, rgb = points_2d(rng, H, W, J), table_2d(rng, J, nb), distinct_colours(rng, J)
    assert bones.shape == (nb, 2)
    for radius in RADII:
        for lw in WIDTHS:
            what = f"radius {radius} line_width {lw}"
            if J >= 19 and nb >= 2 and lw >= 1.0 and radius in (0.5, 3.0):
                # a condition on the INPUTS, read off the oracle's masks: the three ordering rules are exercised in this frame
                bone_masks, joint_masks = orr.pose2d_masks(H, W, pts[0], bones, radius, lw)
                per_bone = np.sum([m for _, m in bone_masks], axis=0)
                per_joint = np.sum([m for _, m in joint_masks], axis=0)
                assert (per_bone >= 2).any(), "no pixel under two bones: choose other inputs"
                assert ((per_bone >= 1) & (per_joint >= 1)).any(), "no pixel under a bone and a joint: choose other inputs"
            got = run_pose2d(native_lib, cuda, luma, pts, bones, rgb, radius, lw)
            ref = orr.pose2d_grid(luma, pts, bones, rgb, radius, lw)
            assert np.array_equal(got, ref), (what, int((got != ref).any(2).sum()))
            for slot in range(6):
                view = got[(slot // 3) * H:(slot // 3 + 1) * H, (slot % 3) * W:(slot % 3 + 1) * W]
                drawing = [j for j in range(J) if _draws(pts[slot, j])]
                if radius == 1e9 and drawing:       # every pixel lies inside every disc: the last joint that draws owns the frame
                    assert (view == rgb[drawing[-1]]).all(), (what, slot)
                if radius == 0.0 and nb == 0:        # exactly the pixels that sit on a joint, the later joint's colour on a shared one
                    want = np.repeat(luma[slot][:, :, None], 3, axis=2)
                    for j in drawing:
                        r, c = pts[slot, j]
                        if r == int(r) and c == int(c) and 0 <= r < H and 0 <= c < W:
                            want[int(r), int(c)] = rgb[j]
                    assert np.array_equal(view, want), (what, slot)


def test_a_joint_that_is_not_finite_draws_nothing_and_disturbs_nothing(native_lib, cuda):
    """The frame with NaN, +Inf, -Inf and 1e300 in single joints equals the frame of the table WITHOUT those joints and their bones."""
    H, W, J = 7, 300, 19
    rng = np.random.default_rng(5)
    luma = rng.integers(0, 256, (6, H, W), dtype=np.uint8)
    pts, rgb = points_2d(rng, H, W, J), distinct_colours(rng, J)
    bad = [10, 11, 12, 13]
    for s in range(6):
        pts[s, 10, 0], pts[s, 11, 1], pts[s, 12, 0], pts[s, 13] = np.nan, np.inf, -np.inf, (1e300, -1e300)
    bones = table_2d(rng, J, 96)
    got = run_pose2d(native_lib, cuda, luma, pts, bones, rgb, 3.0, 2.5)
    clean = pts.copy()
    clean[:, bad] = 0.0   # unseen: neither they nor their bones are drawn
    assert np.array_equal(got, orr.pose2d_grid(luma, clean, bones, rgb, 3.0, 2.5))
    assert np.array_equal(got, run_pose2d(native_lib, cuda, luma, clean, bones, rgb, 3.0, 2.5))


# ---- pose3d ----------------------------------------------------------------------------------------------------------------------------
SIZES_3D = [2, 3, 255, 256, 257]
TABLES_3D = [(1, 0), (1, 96), (38, 0), (38, 96), (64, 0), (64, 96)]
# (lim, azimuths, elevation, line_width, a NaN joint)
VIEWS = [
    (2.0, (0.0, 90.0, -60.0), 30.0, 1.5, False),
    (2.0, (405.0, 120.0, 210.0), 0.0, 1.5, True),
    (2.0, (0.0, 90.0, -60.0), 90.0, 0.0, False),
    (2.0, (-60.0, 405.0, 90.0), -30.0, 1e9, True),
    (1e-3, (0.0, 90.0, 405.0), 30.0, 1.5, False),
    (1e6, (0.0, -60.0, 90.0), 30.0, 1.5, False),
    (0.5, (165.0, -60.0, 0.0), -30.0, 0.0, True),
    (37.5, (405.0, 0.0, 90.0), 90.0, 1.5, False),
    (2.0, (90.0, 0.0, 405.0), 0.0, 1.5, False),
    (1.0, (-60.0, 90.0, 0.0), 30.0, 1e9, False),
]


@pytest.mark.parametrize("J,nb", TABLES_3D, ids=lambda v: str(v))
@pytest.mark.parametrize("size", SIZES_3D)
def test_pose3d_panels_over_sizes_tables_and_views(native_lib, cuda, size, J, nb):
    """Points uniform in +-3 at lim 2 (bones leave the panel), lim from 1e-3 to 1e6, the azimuths 0, 90, -60 and 405, the elevations 0, 30,
    90 and -30, line widths 0, 1.5 and 1e9, a NaN joint.  Panels of 2 and 3 pixels see every view; at 255 .. 257 (the numpy masks of 96
    bones cost a third of a second per frame there) each table sees two of them, and the cases together all ten."""
    case = SIZES_3D.index(size) * len(TABLES_3D) + TABLES_3D.index((J, nb))
    views = VIEWS if size <= 3 or nb == 0 else [VIEWS[(2 * case + k) % len(VIEWS)] for k in range(2)]
    rng = np.random.default_rng(31 * size + J + nb)
    rgb = distinct_colours(rng, J)
    bones = _bones([(0, 0)] * nb if J == 1 else [tuple(int(v) for v in rng.integers(0, J, 2)) for _ in range(nb)])
    drawn = 0
    for lim, az3, elev, lw, nan in views:
        p3 = rng.uniform(-3.0, 3.0, (J, 3))
        if nan:
            p3[J // 2, 1] = np.nan
        got = run_pose3d(native_lib, cuda, p3, bones, rgb, az3, elev, lim, size, lw)
        ref = orr.pose3d_panels(p3, bones, rgb, az3, elev, lim, size, lw)
        assert np.array_equal(got, ref), ((lim, az3, elev, lw, nan), int((got != ref).any(2).sum()))
        if nb == 0:
            assert not got.any()   # the black background, written to every pixel (the buffer held 0xA5)
        drawn += int(got.any(2).sum())
    if nb and J > 1:
        assert drawn > 0   # the comparison is not one of black panels


# ---- resize ----------------------------------------------------------------------------------------------------------------------------
RESIZES = [((1, 1), (5, 7)), ((4, 6), (4, 6)), ((3, 5), (1, 1)), ((2, 300), (3, 257)), ((7, 255), (14, 510)), ((9, 513), (4, 256))]


@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
@pytest.mark.parametrize("src,dst", RESIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_resize_over_sizes_and_pitches(native_lib, cuda, src, dst, pitched):
    rng = np.random.default_rng(src[1] * 7 + dst[1])
    img = np.stack([rng.integers(0, 256, src, dtype=np.uint8), rng.integers(0, 64, src, dtype=np.uint8), 255 - rng.integers(0, 32, src, dtype=np.uint8)], axis=-1)
    got = run_resize(native_lib, cuda, img, *dst, pitched)
    assert np.array_equal(got, orr.resize_rgb(img, *dst))
    if src == dst:
        assert np.array_equal(got, img)   # the identity size is a byte-exact copy


@pytest.mark.parametrize("pitched", [False, True], ids=["contiguous", "pitched"])
def test_resize_rounds_a_half_up(native_lib, cuda, pitched):
    """A 2x up-scale (taps weighted 1/4 and 3/4) of values that differ by 2 between neighbours, along x, along y and along both: the
    value before rounding is k + 0.5 exactly at most pixels, and a kernel that truncated, or rounded half to even, would show."""
    y, x = np.meshgrid(np.arange(6), np.arange(130), indexing="ij")
    img = np.stack([2 * (x % 120), 2 * y + 200, 2 * ((x + y) % 100) + 1], axis=-1)
    assert img.max() <= 255
    img = img.astype(np.uint8)
    raw = orr.resize_rgb(img, 12, 260, unrounded=True)
    halves = raw - np.floor(raw) == 0.5
    assert halves.sum() >= 100, int(halves.sum())
    assert ((np.floor(raw[halves]) % 2) == 0).sum() >= 50 and ((np.floor(raw[halves]) % 2) == 1).sum() >= 50   # both parities: half-to-even differs
    got = run_resize(native_lib, cuda, img, 12, 260, pitched)
    assert np.array_equal(got, orr.resize_rgb(img, 12, 260))
    assert np.array_equal(got[halves], (raw[halves] + 0.5).astype(np.uint8))   # k + 0.5 -> k + 1


# ---- a side stream, twice ----------------------------------------------------------------------------------------------------------------
def test_each_kernel_twice_on_a_side_stream(native_lib, cuda):
    rng = np.random.default_rng(77)
    H, W, J = 5, 513, 64
    luma = rng.integers(0, 256, (6, H, W), dtype=np.uint8)
    pts, bones, rgb = points_2d(rng, H, W, J), table_2d(rng, J, 96), distinct_colours(rng, J)
    p3 = rng.uniform(-3.0, 3.0, (J, 3))
    img = rng.integers(0, 256, (9, 513, 3), dtype=np.uint8)
    side = torch.cuda.Stream(device=cuda)
    runs = []
    for _ in range(2):
        with torch.cuda.stream(side):
            assert _stream(cuda) == side.cuda_stream and side.cuda_stream != 0
            runs.append((run_pose2d(native_lib, cuda, luma, pts, bones, rgb, 3.0, 2.5),
                         run_pose3d(native_lib, cuda, p3, bones, rgb, (0.0, 90.0, -60.0), 30.0, 2.0, 257, 1.5),
                         run_resize(native_lib, cuda, img, 4, 256, True)))
        side.synchronize()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.array_equal(runs[0][0], orr.pose2d_grid(luma, pts, bones, rgb, 3.0, 2.5))
    assert np.array_equal(runs[0][1], orr.pose3d_panels(p3, bones, rgb, (0.0, 90.0, -60.0), 30.0, 2.0, 257, 1.5))
    assert np.array_equal(runs[0][2], orr.resize_rgb(img, 4, 256))


# ---- refusals: DF3D_EINVAL, a message, and no launch ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(cuda):
    """Valid arguments of every call at 4 x 6 pixels and 3 joints, and one guarded output that no refused call may touch."""
    luma = torch.zeros((6, 4, 6), dtype=torch.uint8, device=cuda)
    pts = torch.ones((6, 64, 2), dtype=torch.float64, device=cuda)   # room for every joint count that is tried
    p3 = torch.zeros((64, 3), dtype=torch.float64, device=cuda)
    img = torch.zeros((4, 6, 3), dtype=torch.uint8, device=cuda)
    buf, out_p = _guarded(cuda, 2 * 4 * 3 * 6 * 3)
    return {"luma": luma.data_ptr(), "pts": pts.data_ptr(), "p3": p3.data_ptr(), "img": img.data_ptr(), "buf": buf, "out": out_p,
            "bones": _bones([(0, 1), (1, 2)] + [(0, 0)] * 95), "rgb": distinct_colours(np.random.default_rng(0), 65), "keep": (luma, pts, p3, img)}


def _refused(lib, cuda, small, rc):
    assert rc == EINVAL, rc
    msg = lib.df3d_last_error()
    assert msg and len(msg) > 5, msg
    torch.cuda.synchronize(cuda)
    assert (small["buf"].cpu().numpy() == POISON).all(), "a refused call wrote to its output"


def _pose2d(lib, cuda, s, **kw):
    a = dict(luma=s["luma"], H=4, W=6, pts=s["pts"], J=3, bones=s["bones"], nb=2, rgb=_up(s["rgb"]), radius=3.0, lw=1.0, out=s["out"])
    a.update(kw)
    bones = _ip(a["bones"]) if a["bones"] is not None else None
    with torch.cuda.device(cuda):
        return lib.df3d_render_pose2d_grid(a["luma"], a["H"], a["W"], a["pts"], a["J"], bones, a["nb"], a["rgb"], a["radius"], a["lw"], a["out"], _stream(cuda))


def _pose3d(lib, cuda, s, **kw):
    a = dict(p3=s["p3"], J=3, bones=s["bones"], nb=2, rgb=_up(s["rgb"]), az=(ctypes.c_double * 3)(0.0, 90.0, -60.0), elev=30.0, lim=2.0, size=4, lw=1.5,
             out=s["out"])
    a.update(kw)
    bones = _ip(a["bones"]) if a["bones"] is not None else None
    with torch.cuda.device(cuda):
        return lib.df3d_render_pose3d_panels(a["p3"], a["J"], bones, a["nb"], a["rgb"], a["az"], a["elev"], a["lim"], a["size"], a["lw"], a["out"], _stream(cuda))


def _resize(lib, cuda, s, **kw):
    a = dict(img=s["img"], ih=4, iw=6, ip=6, out=s["out"], oh=4, ow=6, op=6)
    a.update(kw)
    with torch.cuda.device(cuda):
        return lib.df3d_resize_rgb(a["img"], a["ih"], a["iw"], a["ip"], a["out"], a["oh"], a["ow"], a["op"], _stream(cuda))


NAN = float("nan")
BAD_TABLES = [dict(J=0), dict(J=65), dict(nb=97), dict(nb=-1), dict(bones=_bones([(0, 3), (0, 1)])), dict(bones=_bones([(0, 1), (-1, 2)])),
              dict(bones=_bones([(3, 0), (0, 1)])), dict(bones=None), dict(rgb=None)]
BAD_2D = BAD_TABLES + [dict(luma=None), dict(pts=None), dict(out=None), dict(H=0), dict(W=0), dict(H=-1), dict(radius=-1.0), dict(radius=NAN),
                       dict(lw=-0.5), dict(lw=NAN), dict(H=65536), dict(H=65536, W=1)]
BAD_3D = BAD_TABLES + [dict(p3=None), dict(az=None), dict(out=None), dict(lim=0.0), dict(lim=NAN), dict(lim=-2.0), dict(size=1), dict(size=0), dict(lw=-1.0),
                       dict(lw=NAN), dict(size=65536)]
BAD_RESIZE = [dict(img=None), dict(out=None), dict(ih=0), dict(iw=0), dict(oh=0), dict(ow=0), dict(ip=5), dict(op=5), dict(oh=65536), dict(oh=65536, ow=1, op=1)]


def _id(kw):
    return ",".join(f"{k}={'tab' if isinstance(v, np.ndarray) else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD_2D, ids=_id)
def test_pose2d_refuses(native_lib, cuda, small, kw):
    _refused(native_lib, cuda, small, _pose2d(native_lib, cuda, small, **kw))


@pytest.mark.parametrize("kw", BAD_3D, ids=_id)
def test_pose3d_refuses(native_lib, cuda, small, kw):
    _refused(native_lib, cuda, small, _pose3d(native_lib, cuda, small, **kw))


@pytest.mark.parametrize("kw", BAD_RESIZE, ids=_id)
def test_resize_refuses(native_lib, cuda, small, kw):
    _refused(native_lib, cuda, small, _resize(native_lib, cuda, small, **kw))


def test_the_limits_themselves_are_accepted(native_lib, cuda, small):
    """64 joints and 96 bones pass, and so does the valid call the refusals were derived from (the refusals are the arguments' doing)."""
    for call in (_pose2d, _pose3d):
        assert call(native_lib, cuda, small, J=64, nb=96) == 0
        assert call(native_lib, cuda, small, nb=0, bones=None) == 0
    assert _pose2d(native_lib, cuda, small, radius=0.0, lw=0.0) == 0 and _pose3d(native_lib, cuda, small, size=2, lw=0.0) == 0
    assert _resize(native_lib, cuda, small) == 0
    torch.cuda.synchronize(cuda)
    _payload(small["buf"], (2 * 4 * 3 * 6 * 3,))   # the guards around the largest of these frames
    small["buf"].fill_(POISON)


# ---- FrameRenderer's input checks ----------------------------------------------------------------------------------------------------------
# Every wrong tensor is a view into storage at least as large as the right tensor's, on memory the device can read (the "CPU" tensors are
# pinned): were a check missing, the kernel would read or write inside that storage, and the test would fail for the missing ValueError.
H_R, W_R, J_R = 4, 6, 5


def _pinned(shape, dtype):
    return torch.zeros(shape, dtype=dtype).pin_memory()


def _bad_inputs(cuda, shape, dtype, other):
    """name -> a tensor that must be refused where a contiguous `dtype` CUDA tensor of `shape` is expected"""
    n = int(np.prod(shape))
    big = torch.zeros(4 * n * max(torch.empty((), dtype=dtype).element_size(), torch.empty((), dtype=other).element_size()), dtype=torch.uint8, device=cuda)
    typed = big.view(dtype)
    doubled = typed[: 2 * n].view(*shape[:-1], 2 * shape[-1])
    return {
        "dtype": big.view(other)[:n].view(shape),
        "fewer rows": typed[: n // shape[0] * (shape[0] - 1)].view(shape[0] - 1, *shape[1:]) if shape[0] > 1 else typed[: 2 * n].view(2, *shape),
        "more dims": typed[:n].view(1, *shape),
        "narrower": typed[:n].view(shape)[..., : shape[-1] - 1] if shape[-1] > 1 else doubled,
        "strided": doubled[..., ::2],
        "host": _pinned(shape, dtype),
        "no tensor": typed[:n].view(shape).cpu().numpy(),
    }


def test_frame_renderer_checks_its_tensors(native_lib, cuda):
    from deepfly3d_amd import video

    r = video.FrameRenderer(H_R, W_R, J_R, cuda)
    luma = torch.zeros((6, H_R, W_R), dtype=torch.uint8, device=cuda)
    pts = torch.ones((6, J_R, 2), dtype=torch.float64, device=cuda)
    p3 = torch.zeros((J_R, 3), dtype=torch.float64, device=cuda)
    assert r.grid2d(luma, pts).shape == (2 * H_R, 3 * W_R, 3) and r.panels3d(p3, size=4).shape == (4, 12, 3)   # the right ones pass
    out2, out3 = torch.zeros((2 * H_R, 3 * W_R, 3), dtype=torch.uint8, device=cuda), torch.zeros((4, 12, 3), dtype=torch.uint8, device=cuda)
    assert r.grid2d(luma, pts, out=out2) is out2 and r.panels3d(p3, out=out3, size=4) is out3
    for name, bad in _bad_inputs(cuda, (6, H_R, W_R), torch.uint8, torch.float32).items():
        with pytest.raises(ValueError, match="luma6"):
            r.grid2d(bad, pts)
    for name, bad in _bad_inputs(cuda, (6, J_R, 2), torch.float64, torch.float32).items():
        with pytest.raises(ValueError, match="points6"):
            r.grid2d(luma, bad)
    for name, bad in _bad_inputs(cuda, (2 * H_R, 3 * W_R, 3), torch.uint8, torch.int8).items():
        with pytest.raises(ValueError, match="out"):
            r.grid2d(luma, pts, out=bad)
    for name, bad in _bad_inputs(cuda, (J_R, 3), torch.float64, torch.float32).items():
        with pytest.raises(ValueError, match="points3d"):
            r.panels3d(bad, size=4)
    for name, bad in _bad_inputs(cuda, (4, 12, 3), torch.uint8, torch.int8).items():
        with pytest.raises(ValueError, match="out"):
            r.panels3d(p3, out=bad, size=4)
    # a renderer of another joint count or frame size refuses what the first one took
    with pytest.raises(ValueError, match="points6"):
        video.FrameRenderer(H_R, W_R, J_R + 1, cuda).grid2d(luma, pts)
    with pytest.raises(ValueError, match="luma6"):
        video.FrameRenderer(H_R, W_R + 1, J_R, cuda).grid2d(luma, pts)
    with pytest.raises(ValueError, match="points3d"):
        video.FrameRenderer(H_R, W_R, J_R + 1, cuda).panels3d(p3)


def test_frame_renderer_resize_checks_its_images(native_lib, cuda):
    from deepfly3d_amd import video

    r = video.FrameRenderer(H_R, W_R, J_R, cuda)
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    wide_in = torch.from_numpy(rng.integers(0, 256, (9, 20, 3), dtype=np.uint8)).to(cuda)
    wide_in[:, 2:15] = torch.from_numpy(src).to(cuda)
    frame = torch.full((12, 30, 3), POISON, dtype=torch.uint8, device=cuda)
    got = r.resize(wide_in[:, 2:15], frame[3:8, 4:11])    # views of wider images on both sides: pitches from the strides
    assert got.data_ptr() == frame[3:8, 4:11].data_ptr()
    want = np.full((12, 30, 3), POISON, np.uint8)
    want[3:8, 4:11] = orr.resize_rgb(src, 5, 7)
    assert np.array_equal(frame.cpu().numpy(), want)
    img, out = torch.zeros((4, 6, 3), dtype=torch.uint8, device=cuda), torch.zeros((5, 7, 3), dtype=torch.uint8, device=cuda)
    four = torch.zeros((8, 8, 4), dtype=torch.uint8, device=cuda)
    bad = {
        "dtype": torch.zeros((4, 6, 3), dtype=torch.float32, device=cuda),
        "two dims": torch.zeros((4, 18), dtype=torch.uint8, device=cuda),
        "four channels": four[:4, :6],
        "pixels of four bytes": four[:4, :6, :3],
        "every other pixel": torch.zeros((4, 12, 3), dtype=torch.uint8, device=cuda)[:, ::2],
        "transposed": torch.zeros((6, 4, 3), dtype=torch.uint8, device=cuda).transpose(0, 1),
        "a pitch of no whole pixels": torch.zeros((4 * 20,), dtype=torch.uint8, device=cuda).as_strided((4, 6, 3), (20, 3, 1)),
        "rows that overlap": torch.zeros((4 * 18,), dtype=torch.uint8, device=cuda).as_strided((4, 6, 3), (15, 3, 1)),
        "empty": torch.zeros((0, 6, 3), dtype=torch.uint8, device=cuda),
        "host": _pinned((4, 6, 3), torch.uint8),
        "no tensor": np.zeros((4, 6, 3), np.uint8),
    }
    for name, t in bad.items():
        with pytest.raises(ValueError, match="img"):
            r.resize(t, out)
        with pytest.raises(ValueError, match="out"):
            r.resize(img, t)
