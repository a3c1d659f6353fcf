"""Every plan step of the default fp32 engine (Winograd tails: csrc/hg_bt_wino_f32.h, hg_l1_wino_f32.h), pinned bit for bit.

tests/test_gpu_bt_pinned.py pins the final heat-maps; a wrong value that a later ReLU or max-pool swallows passes there.  Here the output tensor
of EVERY plan step is hashed (forward_upto on a NaN-poisoned workspace: a step that reads memory this forward has not written shows it), so a
change to those kernels' scheduling or addressing that moves one value of one block is seen at the block that produced it.

  * the input is seeded, 64 x 192 (quarter-resolution bottleneck tiles 2 x 3, half-resolution layer1 tiles 4 x 3 per view), at V = 1 and at the
    V of test_gpu_bt_pinned.many_views (every persistent grid ends on a partial round);
  * options {}, fuse_upadd = 1, 2 and False: together the plain, ADD2 and UP identity tails, layer2's and layer1's Winograd kernels all run.

The digests in tests/golden/hg_wino_step_digests.json were recorded with `python tests/test_gpu_wino_steps_pinned.py` (on the GPU) with the
library of the commit before this test was added (round 7's kernels, before their phase-2 addressing was rewritten), twice in two processes
that agreed; "cu" is the compute-unit count of the recording device (the larger V follows from it)."""
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_gpu_bt_pinned import BT_H, BT_TILES, BT_W, many_ok, many_views   # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "hg_wino_step_digests.json")
# append only: a case's input seed is its position in CASES
OPTIONS = [{}, {"fuse_upadd": 1}, {"fuse_upadd": 2}, {"fuse_upadd": False}]
CASES = [(o, v) for o in range(len(OPTIONS)) for v in ("one", "many")]


def case_name(c):
    return " ".join(["f32"] + [f"{k}={int(v)}" for k, v in OPTIONS[c[0]].items()] + [c[1]])


def step_digests(case, engines, device, cu):
    """engines: index into OPTIONS -> HourglassEngine, filled here.  Returns [[step name, sha256 of its output tensor], ...] in plan order."""
    import torch

    from deepfly3d_amd.hourglass import HourglassEngine
    from deepfly3d_amd.synthetic import synthetic_state_dict

    if case[0] not in engines:
        engines[case[0]] = HourglassEngine(synthetic_state_dict(3), dtype="f32", device=device, height=BT_H, width=BT_W, **OPTIONS[case[0]])
    eng = engines[case[0]]
    views = 1 if case[1] == "one" else many_views(cu)
    if case[1] == "many":
        assert many_ok(views * BT_TILES, cu), (views, cu)
    g = torch.Generator().manual_seed(7100 + CASES.index(case))
    images = (torch.rand((views, BT_H, BT_W, 3), generator=g) * 2.0 - 0.75).to(device)
    out = []
    for k, (name, _) in enumerate(eng.steps(), start=1):
        eng._workspace(views).fill_(0xFF)
        t = eng.forward_upto(images, k).contiguous().cpu().numpy()
        out.append([f"{k} {name}", hashlib.sha256(t.tobytes()).hexdigest()])
    return out


@pytest.fixture(scope="module")
def engines():
    return {}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert sorted(fx["digests"]) == sorted(case_name(c) for c in CASES)
    return fx


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_name)
def test_every_plan_step_is_unchanged(cuda, engines, recorded, case):
    import torch

    name = case_name(case)
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    if case[1] == "many" and cu != recorded["cu"]:
        pytest.skip(f"{name}: the view count follows from the CU count; recorded on {recorded['cu']} CUs, this device has {cu}")
    got = step_digests(case, engines, cuda, cu)
    want = recorded["digests"][name]
    assert [s for s, _ in got] == [s for s, _ in want], f"{name}: the plan changed"
    changed = [s for (s, a), (_, b) in zip(got, want) if a != b]
    assert not changed, f"{name}: the output of step(s) {changed} changed (the first one is where to look)"


if __name__ == "__main__":
    import torch

    sys.path.insert(0, os.path.dirname(HERE))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    engines = {}
    fx = {"cu": cu, "digests": {case_name(c): step_digests(c, engines, dev, cu) for c in CASES}}
    with open(out, "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")
    print(out, cu, hashlib.sha256(json.dumps(fx, sort_keys=True).encode()).hexdigest())
