"""The bytes df3d_hg_set_weights writes behind the engine's plan, pinned: the plan's stream offsets and sizes and the packers' grids must
keep agreeing.  The heat-maps alone cannot show that -- a stream misplaced into a slot that happens to be unread leaves them right.

Each engine's buffer is filled with 0xA5 and packed again, so the bytes no packer writes (the unused halves of stage images, reserved
slots) are deterministic and a packer that starts writing where it did not before is caught too.  The digests in
tests/golden/hg_lowp_digests.json were recorded with `python tests/test_gpu_hg_weight_streams.py` (on the GPU)."""
import hashlib
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hg_lowp_digests.json")
ENGINES = [("f32", {}), ("f32", {"wino": 0}), ("f32", {"split1": 0}), ("f32s", {}), ("bf16", {}), ("bf16", {"w2d": 0}), ("f16", {})]


def engine_name(e):
    return " ".join([e[0]] + [f"{k}={v}" for k, v in e[1].items()]) if e[1] else f"{e[0]} default"


def lowp_digest(dtype, options, state_dict, device):
    import torch

    from deepfly3d_amd import _native
    from deepfly3d_amd.hourglass import HourglassEngine

    eng = HourglassEngine(state_dict, dtype=dtype, device=device, height=64, width=64, **options)
    assert eng.lowp is not None and eng.lowp.numel() == eng.lib.df3d_hg_lowp_bytes(eng.h)
    eng.lowp.fill_(0xA5)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        _native.check(eng.lib.df3d_hg_set_weights(eng.h, eng.blob.data_ptr(), eng.lowp.data_ptr(), stream), "df3d_hg_set_weights")
    torch.cuda.synchronize(device)
    return hashlib.sha256(eng.lowp.cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def state_dict():
    from deepfly3d_amd.synthetic import synthetic_state_dict

    return synthetic_state_dict(0)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES, ids=engine_name)
def test_weight_streams_are_unchanged(cuda, state_dict, engine):
    with open(FIXTURE) as f:
        want = json.load(f)[engine_name(engine)]
    got = lowp_digest(engine[0], engine[1], state_dict, cuda)
    assert got == want, f"{engine_name(engine)}: the packed weight buffer changed"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deepfly3d_amd.synthetic import synthetic_state_dict

    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    sd = synthetic_state_dict(0)
    digests = {engine_name(e): lowp_digest(e[0], e[1], sd, "cuda:0") for e in ENGINES}
    with open(out, "w") as f:
        json.dump(digests, f, indent=1)
        f.write("\n")
    print(json.dumps(digests, indent=1))
