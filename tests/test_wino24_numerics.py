"""CPU gate for the fp32 bottleneck tail's Winograd F(2x4, 3x3) (deepfly3d_amd/csrc/hg_bt_wino_f32.h): the transform matrices in exact
rationals, and one fused identity tail emulated in float32 in the kernel's order of operations, scored the way oracle/hg_local.py scores
a float32 step (max |got - ref| / (2^-24 scale)).  No GPU."""
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hourglass_torch as oh
from oracle.hg_local import FP32_ERR

# F(4, 3), points (0, 1, -1, 1/2, -2, inf): what bt_wino_pack_kernel (G) and the kernel's transforms (B^T, A^T) use
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, Fr(1, 2), -2, 0], [0, 1, 1, Fr(1, 4), 4, 0], [0, 1, -1, Fr(1, 8), -8, 1]]
BT4 = [[1, Fr(-3, 2), -2, Fr(3, 2), 1, 0], [0, -1, Fr(1, 2), Fr(5, 2), 1, 0], [0, 1, Fr(-5, 2), Fr(1, 2), 1, 0],
       [0, -2, -1, 2, 1, 0], [0, Fr(1, 2), -1, Fr(-1, 2), 1, 0], [0, 1, Fr(-3, 2), -2, Fr(3, 2), 1]]
G4 = [[1, 0, 0], [Fr(1, 3), Fr(1, 3), Fr(1, 3)], [Fr(-1, 3), Fr(1, 3), Fr(-1, 3)], [Fr(-16, 15), Fr(-8, 15), Fr(-4, 15)],
      [Fr(1, 15), Fr(-2, 15), Fr(4, 15)], [0, 0, 1]]
# F(2, 3), points (0, 1, -1, inf)
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G2 = [[1, 0, 0], [Fr(1, 2), Fr(1, 2), Fr(1, 2)], [Fr(1, 2), Fr(-1, 2), Fr(1, 2)], [0, 0, 1]]


def _exact_1d(AT, BT, G, m):
    """A^T [(G g) (.) (B^T d)] == the 1-D correlation y_k = sum_t g_t d_{k+t}, symbolically: every (g_t, d_s) coefficient."""
    n = m + 2
    for k in range(m):
        for t in range(3):
            for s in range(n):
                c = sum(Fr(AT[k][p]) * Fr(G[p][t]) * Fr(BT[p][s]) for p in range(n))
                assert c == (1 if s == k + t else 0), (m, k, t, s, c)


def test_transforms_exact():
    _exact_1d(AT4, BT4, G4, 4)
    _exact_1d(AT2, BT2, G2, 2)
    # B^T and A^T are exact in float32 (the kernel builds V and Y with them); G's thirds and fifteenths go into U, rounded once from fp64
    for M in (AT4, BT4, AT2, BT2):
        for row in M:
            for v in row:
                assert Fr(float(np.float32(float(v)))) == Fr(v)


def _f(M):
    return np.array([[float(v) for v in r] for r in M], dtype=np.float64)


def _bt4_f32(x):
    """The kernel's F(4, 3) input transform on the last axis (6 values), float32, its order of operations."""
    x0, x1, x2, x3, x4, x5 = (x[..., i] for i in range(6))
    h = np.float32(0.5)
    d13 = x3 - x1
    v0 = (x0 + x4) - 2 * x2 + d13 + h * d13
    v1 = (x4 - x1) + h * x2 + 2 * x3 + h * x3
    v2 = (x4 + x1) - 2 * x2 - h * x2 + h * x3
    v3 = (x4 - x2) + 2 * (x3 - x1)
    v4 = (x4 - x2) + h * (x1 - x3)
    d24 = x4 - x2
    v5 = (x5 + x1) - 2 * x3 + d24 + h * d24
    return np.stack([v0, v1, v2, v3, v4, v5], axis=-1).astype(np.float32)


def _at4_f32(s):
    s0, s1, s2, s3, s4, s5 = (s[..., i] for i in range(6))
    a, b = s1 + s2, s1 - s2
    y0 = s0 + a + s3 + s4
    y1 = b + np.float32(0.5) * s3 - 2 * s4
    y2 = a + np.float32(0.25) * s3 + 4 * s4
    y3 = b + np.float32(0.125) * s3 - 8 * s4 + s5
    return np.stack([y0, y1, y2, y3], axis=-1).astype(np.float32)


def wino24_tail_f32(t1, x, w2, b2, w3, b3):
    """One fused identity tail (3x3 -> + b2 -> ReLU -> 1x1 -> + b3 + x), 3x3 as F(2x4, 3x3), float32.  t1 [C, H, W], x [Co, H, W]."""
    C, H, W = t1.shape
    # U = G2 g G4^T in fp64, rounded once: [cout][cin][4][6]
    U = np.einsum("ia,ocab,jb->ocij", _f(G2), w2, _f(G4)).astype(np.float32)
    tp = np.zeros((C, H + 2, W + 2), np.float32)
    tp[:, 1:-1, 1:-1] = t1
    ph, pw = H // 2, W // 4
    # patches d [C][ph][pw][4][6]
    d = np.stack([np.stack([tp[:, 2 * r: 2 * r + 4, 4 * c: 4 * c + 6] for c in range(pw)], 1) for r in range(ph)], 1)
    # rows (F(2,3) direction) first, then columns
    r0 = d[..., 0, :] - d[..., 2, :]
    r1 = d[..., 1, :] + d[..., 2, :]
    r3 = d[..., 1, :] - d[..., 3, :]
    r2 = d[..., 2, :] - d[..., 1, :]
    V = _bt4_f32(np.stack([r0, r1, r2, r3], -2))                          # [C][ph][pw][4][6]
    M = np.einsum("ocij,cpqij->opqij", U, V.astype(np.float32)).astype(np.float32)   # float32 products, float32 sums (BLAS order)
    M[..., 1, 1] += b2[:, None, None].astype(np.float32)
    s0 = M[..., 0, :] + M[..., 1, :] + M[..., 2, :]
    s1 = M[..., 1, :] - M[..., 2, :] - M[..., 3, :]
    Y = _at4_f32(np.stack([s0, s1], -2))                                   # [Co][ph][pw][2][4]
    t2 = np.maximum(Y.transpose(0, 1, 3, 2, 4).reshape(-1, H, W), 0).astype(np.float32)
    out = (np.einsum("oc,chw->ohw", w3.astype(np.float32), t2).astype(np.float32) + b3[:, None, None].astype(np.float32)) + x
    return out.astype(np.float32)


def test_wino24_fused_tail_score():
    """The go / no-go figure: the worst hg_local-style score of one fused identity tail must be at most half the bound."""
    net = oh.build(0)
    g = torch.Generator().manual_seed(0)
    img = torch.rand((1, 256, 512, 3), generator=g)
    rec = oh.forward_traced(net, img)
    name = "hg.0.hg.3.0.0"   # the top level's first plain identity block: 64 x 128, 256 -> 128 -> 128 -> 256
    t1 = rec[name + ".conv1"][0].permute(2, 0, 1).contiguous().numpy().astype(np.float32)
    x = rec["layer3.0.conv3"][0].permute(2, 0, 1).contiguous().numpy().astype(np.float32)
    with torch.no_grad():
        convs, _ = oh._folded(net)
    w2, b2 = (v.detach().numpy() for v in convs[name + ".conv2"])
    w3, b3 = (v.detach().numpy() for v in convs[name + ".conv3"])
    got = wino24_tail_f32(t1, x, w2, b2, w3[:, :, 0, 0], b3)
    # float64 reference and scale: the layer on magnitudes, as oracle/hourglass_torch.forward_traced records for conv3 of a fused block
    T1, X = torch.from_numpy(t1).double()[None], torch.from_numpy(x).double()[None]
    t2 = F.conv2d(T1, torch.from_numpy(w2), torch.from_numpy(b2), padding=1).clamp_min(0)
    ref = F.conv2d(t2, torch.from_numpy(w3), torch.from_numpy(b3)) + X
    scale = F.conv2d(t2.abs(), torch.from_numpy(w3).abs(), torch.from_numpy(b3).abs()) + X.abs()
    err = float(((torch.from_numpy(got).double()[None] - ref).abs() / (2.0**-24 * scale)).max())
    print(f"F(2x4, 3x3) fused identity tail, {name}: worst local figure {err:.2f} (bound {FP32_ERR['wino']})")
    assert err <= FP32_ERR["wino"] / 2, err
