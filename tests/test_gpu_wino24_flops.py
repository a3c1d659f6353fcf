"""-m gpu: the executed-FLOP accounting of the fp32 Winograd tails (df3d_hg_profile_executed_flops).  The bottleneck tail's 3x3 runs as
F(2x4, 3x3) -- 24 products per 2 x 4 output patch and (cin, cout) pair, 3 per pixel against the direct form's 9 -- and layer1's as F(2x2, 3x3)
(4 per pixel); the 1x1 convolutions are executed as they are.  One forward of one view at 256 x 512."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_wino_tail_executed_flops(native_lib, cuda):
    from deepfly3d_amd import _native
    from deepfly3d_amd.hourglass import HourglassEngine
    from deepfly3d_amd.synthetic import synthetic_state_dict

    lib = _native.load()
    dev = torch.device("cuda:0")
    eng = HourglassEngine(synthetic_state_dict(0), dtype="f32", device=dev)
    frames = torch.rand((1, 256, 512, 3), generator=torch.Generator().manual_seed(0)).to(dev)
    eng.forward(frames)   # (first launches: attributes, code objects)
    torch.cuda.synchronize()
    _native.check(lib.df3d_hg_profile(eng.h, 1))
    eng.forward(frames)
    torch.cuda.synchronize()
    # executed / direct per kernel, the executed side counted from the kernels' MFMA instructions per wave and tile (4 waves per tile):
    #   bottleneck tail, 8 x 16 tile: phase 2 = 16 chunks x 6 passes x 16 v_mfma_f32_16x16x4_f32 (2 * 16 * 16 * 4 FLOP), phase 3 = W3
    #   (256 x 128) as 512 v_mfma_f32_32x32x2_f32 (2 * 32 * 32 * 2 FLOP), layer2 another 512 for Wd (256 x 128);
    #   layer1, 8 x 32 tile: phase 2 = 8 chunks x 4 K pairs x 16 positions of v_mfma_f32_32x32x2_f32, phase 3 = W3 and Wd (128 x 64 each) as 512
    # the direct side as the engine reports it: 2 px (9 pl^2 + 2 pl^2 (+ 2 cin pl)), pl = planes, cin = the block's input channels
    F16, F32 = 2 * 16 * 16 * 4, 2 * 32 * 32 * 2
    tail = 4 * (16 * 6 * 16 * F16 + 512 * F32) / (2.0 * 128 * (9 + 2) * 128 * 128)
    l2 = 4 * (16 * 6 * 16 * F16 + 1024 * F32) / (2.0 * 128 * (9 * 128 * 128 + 2 * 128 * 128 + 128 * 2 * 128))
    l1 = 4 * (8 * 4 * 16 * F32 + 512 * F32) / (2.0 * 256 * (9 * 64 * 64 + 2 * 64 * 64 + 64 * 2 * 64))
    want = {"bottleneck_wino_f32_kernel<false, false, false>": tail,
            "bottleneck_wino_f32_kernel<false, true, false>": tail,
            "bottleneck_wino_f32_kernel<true, false, false>": tail,
            "bottleneck_wino_f32_kernel<false, false, true>": l2,
            "layer1_wino_f32_kernel": l1}
    seen = {}
    buf = ctypes.create_string_buffer(128)
    for k in range(lib.df3d_hg_profile_count(eng.h)):
        ms, fl, by, m1, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _native.check(lib.df3d_hg_profile_read(eng.h, k, buf, 128, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(m1), ctypes.byref(n)))
        ex = ctypes.c_double()
        _native.check(lib.df3d_hg_profile_executed_flops(eng.h, k, ctypes.byref(ex)))
        name = buf.value.decode()
        if n.value and name in want:
            seen[name] = ex.value / fl.value
    _native.check(lib.df3d_hg_profile(eng.h, 0))
    assert set(seen) == set(want), sorted(seen)
    for name, r in seen.items():
        assert abs(r - want[name]) < 1e-12, (name, r, want[name])
