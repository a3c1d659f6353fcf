"""numpy statement of the baseline JPEG encoder of DESIGN.md section 27 (libjpeg's rules: integer colour conversion, 4:2:0 with the
h2v2 downsampler's alternating bias, the "islow" forward DCT, division by 8 q, the Annex K Huffman tables, no restart markers).

Every stage is exposed, so that a test can tell which rule a kernel broke:

    planes(rgb)                  -> y, cb, cr          the padded component planes
    coefficients(rgb, quality)   -> [blocks, 64] int16 quantised, zigzag order, blocks in scan order (per MCU: Y00 Y01 Y10 Y11 Cb Cr),
                                                       dummy blocks filled by libjpeg's rule
    block_bits(coef)             -> [blocks] int64     entropy-coded bits of every block
    unstuffed(coef)              -> bytes              the bit stream, last byte padded with 1-bits
    scan(coef)                   -> bytes              with a zero byte after every 0xFF
    header(width, height, quality), file(rgb, quality)

Independent of the package: it shares no table and no line with deepfly3d_amd/jpeg.py.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])


def _codes(spec):
    """(bits, values) -> {symbol: (code, length)}: canonical codes, Annex C."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (_codes(DC_LUMA), _codes(DC_CHROMA))
AC_CODES = (_codes(AC_LUMA), _codes(AC_CHROMA))


def quality_tables(quality):
    """Two [64] arrays, natural order."""
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def _ceil(a, b):
    return -(-a // b)


def planes(rgb):
    """[H, W, 3] uint8 -> (y [8 ceil(H/8), 8 ceil(W/8)], cb, cr [8 ceil(H/16), 8 ceil(W/16)]) int64, in 0 .. 255."""
    rgb = np.asarray(rgb).astype(np.int64)
    H, W, _ = rgb.shape
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    y = np.pad(y, ((0, 8 * _ceil(H, 8) - H), (0, 8 * _ceil(W, 8) - W)), mode="edge")

    def down(c):
        c = np.pad(c, ((0, H & 1), (0, 16 * _ceil(W, 16) - W)), mode="edge")
        bias = np.tile([1, 2], c.shape[1] // 4)[None, :]
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        return np.pad(d, ((0, 8 * _ceil(H, 16) - d.shape[0]), (0, 0)), mode="edge")

    return y, down(cb), down(cr)


_FIX = {name: int(round(c * 8192)) for name, c in dict(
    f0_298=0.298631336, f0_390=0.390180644, f0_541=0.541196100, f0_765=0.765366865, f0_899=0.899976223, f1_175=1.175875602, f1_501=1.501321110,
    f1_847=1.847759065, f1_961=1.961570560, f2_053=2.053119869, f2_562=2.562915447, f3_072=3.072711026).items()}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """d: eight arrays (the samples of one row or column, for every block); the pass of jfdctint."""
    F = _FIX
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * F["f0_541"]
    out[2] = _descale(z1 + t13 * F["f0_765"], n)
    out[6] = _descale(z1 - t12 * F["f1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["f1_175"]
    t4, t5, t6, t7 = t4 * F["f0_298"], t5 * F["f2_053"], t6 * F["f3_072"], t7 * F["f1_501"]
    z1, z2, z3, z4 = -z1 * F["f0_899"], -z2 * F["f2_562"], -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return out


def fdct(blocks):
    """[..., 8, 8] samples (0 .. 255) -> [..., 8, 8] int64, 8 x the DCT of (samples - 128)."""
    x = np.asarray(blocks).astype(np.int64) - 128
    rows = np.stack(_dct_pass([x[..., :, k] for k in range(8)], True), axis=-1)
    return np.stack(_dct_pass([rows[..., k, :] for k in range(8)], False), axis=-2)


def _quantise(c, table):
    d = 8 * table.reshape(8, 8)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def _blocks_of(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)     # [rows, cols, 8, 8]


def coefficients(rgb, quality):
    """[blocks, 64] int16: quantised coefficients in zigzag order, blocks in scan order, dummy blocks by libjpeg's rule."""
    H, W, _ = np.asarray(rgb).shape
    ql, qc = quality_tables(quality)
    y, cb, cr = planes(rgb)
    qy = _quantise(fdct(_blocks_of(y)), ql).reshape(_ceil(H, 8), _ceil(W, 8), 64)[..., ZIGZAG]
    qcb = _quantise(fdct(_blocks_of(cb)), qc).reshape(_ceil(H, 16), _ceil(W, 16), 64)[..., ZIGZAG]
    qcr = _quantise(fdct(_blocks_of(cr)), qc).reshape(_ceil(H, 16), _ceil(W, 16), 64)[..., ZIGZAG]
    out = []
    for my in range(_ceil(H, 16)):
        for mx in range(_ceil(W, 16)):
            for by in range(2):
                for bx in range(2):
                    gy, gx = 2 * my + by, 2 * mx + bx
                    if gy < qy.shape[0] and gx < qy.shape[1]:
                        out.append(qy[gy, gx])
                    else:                       # a dummy block: no AC, the DC of the block before it in the MCU
                        blk = np.zeros(64, np.int64)
                        blk[0] = out[-1][0]
                        out.append(blk)
            out.append(qcb[my, mx])
            out.append(qcr[my, mx])
    return np.asarray(out).astype(np.int16)


def _size(v):
    return int(abs(int(v))).bit_length()


def _block_symbols(blk, diff, comp):
    """[(bits, length), ...] of one block."""
    tab = 0 if comp == 0 else 1
    s = _size(diff)
    assert s <= 11
    out = [DC_CODES[tab][s]]
    if s:
        out.append(((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s))
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(AC_CODES[tab][0xF0])
            run -= 16
        s = _size(v)
        assert s <= 10
        out.append(AC_CODES[tab][(run << 4) | s])
        out.append(((v if v >= 0 else v - 1) & ((1 << s) - 1), s))
        run = 0
    if run:
        out.append(AC_CODES[tab][0x00])
    return out


def _symbols(coef):
    coef = np.asarray(coef)
    pred = [0, 0, 0]
    for i, blk in enumerate(coef):
        comp = (0, 0, 0, 0, 1, 2)[i % 6]
        dc = int(blk[0])
        yield _block_symbols(blk, dc - pred[comp], comp)
        pred[comp] = dc


def block_bits(coef):
    return np.array([sum(length for _, length in syms) for syms in _symbols(coef)], dtype=np.int64)


def unstuffed(coef):
    acc, nbits = 0, 0
    for syms in _symbols(coef):
        for bits, length in syms:
            acc = (acc << length) | bits
            nbits += length
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((nbits + pad) // 8, "big")


def scan(coef):
    return unstuffed(coef).replace(b"\xff", b"\xff\x00")


def header(width, height, quality):
    ql, qc = quality_tables(quality)

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist())) + seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    out += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))


def file(rgb, quality):
    H, W, _ = np.asarray(rgb).shape
    return header(W, H, quality) + scan(coefficients(rgb, quality)) + b"\xff\xd9"
