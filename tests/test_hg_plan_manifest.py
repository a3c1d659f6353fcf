"""The hourglass engine's plan, pinned: what the plan entry points of the C ABI report for every dtype and every plan-changing option
must equal tests/golden/hg_plan_manifest.json, and every refusal of df3d_hg_set_option must keep its text.  No device is needed: the
plan is host code.

The four default manifests (256 x 512, two stacks) are stored readably, every other one as the SHA-256 of its canonical JSON.
`python tests/test_hg_plan_manifest.py` rewrites the fixture (after a deliberate change of the plan)."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hg_plan_manifest.json")
DTYPES = {"f32": 0, "bf16": 1, "f16": 2, "f32s": 3}   # DF3D_DTYPE_* of include/df3d_hip.h
CONFIGS = [(), ("fuse", 0), ("fuse_upadd", 0), ("fuse_upadd", 2), ("ring", 0), ("l1", 0), ("w2d", 0), ("split1", 0), ("split1", 9), ("split1", 10),
           ("split1", 12), ("wino", 0), ("no_reuse", 1), ("chain_views", 2)]
INPUTS = [(256, 512), (64, 64)]
STACKS = [1, 2]
DEFAULT_SHAPE = ((256, 512), 2)   # the manifests kept readably
VIEWS = 3
# (key, value) that df3d_hg_set_option must refuse with DF3D_EINVAL
BAD_VALUES = [("fuse", 2), ("fuse", -1), ("fuse_upadd", 3), ("fuse_upadd", -1), ("l1", 2), ("ring", 2), ("w2d", 2), ("ring2", 2), ("split1", 2),
              ("split1", 7), ("split1", 16), ("split1", -1), ("wino", 2), ("c1res", 2), ("no_reuse", 2), ("chain_views", -1), ("row_bytes", 32),
              ("row_bytes", 256), ("no_such_option", 0)]
# (key, value) in range, tried once weights are set: the options that change the plan are refused, the others accepted
AFTER_WEIGHTS = [("fuse", 1), ("fuse_upadd", 1), ("l1", 1), ("ring", 0), ("w2d", 1), ("ring2", 0), ("split1", 1), ("wino", 1), ("c1res", 0),
                 ("no_reuse", 0), ("chain_views", 0), ("chain_views", 4), ("row_bytes", 64)]
DF3D_EINVAL = -1


def config_name(cfg):
    return "=".join(map(str, cfg)) if cfg else "defaults"


def create(lib, dtype, stacks, hw, cfg):
    h = ctypes.c_void_p()
    assert lib.df3d_hg_create(DTYPES[dtype], stacks, ctypes.byref(h)) == 0
    assert lib.df3d_hg_set_input(h, *hw) == 0
    if cfg:
        assert lib.df3d_hg_set_option(h, cfg[0].encode(), cfg[1]) == 0, lib.df3d_last_error()
    return h


def manifest(lib, dtype, stacks, hw, cfg):
    from deepfly3d_amd import _native

    h = create(lib, dtype, stacks, hw, cfg)
    buf, hwc = ctypes.create_string_buffer(96), (ctypes.c_int * 3)()
    steps = []
    for i in range(lib.df3d_hg_num_steps(h)):
        assert lib.df3d_hg_step_desc(h, i, buf, 96, hwc) == 0
        steps.append([buf.value.decode(), list(hwc), lib.df3d_hg_step_m1_bytes(h, i, VIEWS)])
    d = _native.HGParam()
    params = []
    for i in range(lib.df3d_hg_num_params(h)):
        assert lib.df3d_hg_param_desc(h, i, ctypes.byref(d)) == 0
        params.append([d.name.decode()] + [int(getattr(d, f)) for f, _ in _native.HGParam._fields_[1:]])
    flops, nbytes = ctypes.c_double(), ctypes.c_double()
    assert lib.df3d_hg_work(h, VIEWS, ctypes.byref(flops), ctypes.byref(nbytes)) == 0
    m = {
        "num_steps": lib.df3d_hg_num_steps(h),
        "steps": steps,   # name, hwc, df3d_hg_step_m1_bytes(step, 3)
        "workspace_bytes": lib.df3d_hg_workspace_bytes(h, VIEWS),
        "lowp_bytes": lib.df3d_hg_lowp_bytes(h),
        "blob_floats": lib.df3d_hg_blob_floats(h),
        "param_fields": [f for f, _ in _native.HGParam._fields_],
        "params": params,
        "work": [flops.value, nbytes.value],   # df3d_hg_work(h, 3): flops, bytes
    }
    lib.df3d_hg_destroy(h)
    return m


def digest(m):
    return hashlib.sha256(json.dumps(m, sort_keys=True).encode()).hexdigest()


def shape_key(dtype, cfg, hw, stacks):
    return f"{dtype}/{config_name(cfg)}/{hw[0]}x{hw[1]}/stacks={stacks}"


def option_errors(lib):
    """The text of every refusal: out-of-range values and an unknown key on a fresh engine, then every option on an engine with weights."""
    out = {}
    h = create(lib, "f32", 2, (64, 64), ())
    for key, value in BAD_VALUES:
        assert lib.df3d_hg_set_option(h, key.encode(), value) == DF3D_EINVAL, (key, value)
        out[f"{key}={value}"] = lib.df3d_last_error().decode()
    for args in [(None, b"fuse", 0), (h, None, 0)]:
        assert lib.df3d_hg_set_option(*args) == DF3D_EINVAL
    out["null argument"] = lib.df3d_last_error().decode()
    # weights: an f32 engine without a stream buffer plans itself without weight streams and touches no device
    assert lib.df3d_hg_set_option(h, b"chain_views", 2) == 0
    blob = np.zeros(lib.df3d_hg_blob_floats(h) + 64, dtype=np.float32)
    ptr = (blob.ctypes.data + 255) & ~255
    assert lib.df3d_hg_set_weights(h, ptr, None, None) == 0, lib.df3d_last_error()
    for key, value in AFTER_WEIGHTS:
        rc = lib.df3d_hg_set_option(h, key.encode(), value)
        assert rc in (0, DF3D_EINVAL)
        out[f"after weights: {key}={value}"] = lib.df3d_last_error().decode() if rc else "accepted"
    lib.df3d_hg_destroy(h)
    return out


def record(lib):
    fx = {"defaults": {}, "sha256": {}, "errors": option_errors(lib)}
    for dtype in DTYPES:
        for cfg in CONFIGS:
            for hw in INPUTS:
                for stacks in STACKS:
                    m = manifest(lib, dtype, stacks, hw, cfg)
                    if not cfg and (hw, stacks) == DEFAULT_SHAPE:
                        fx["defaults"][dtype] = m
                    else:
                        fx["sha256"][shape_key(dtype, cfg, hw, stacks)] = digest(m)
    return fx


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("cfg", CONFIGS, ids=config_name)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_plan_manifest_is_unchanged(native_lib, fixture, dtype, cfg):
    for hw in INPUTS:
        for stacks in STACKS:
            m = manifest(native_lib, dtype, stacks, hw, cfg)
            if not cfg and (hw, stacks) == DEFAULT_SHAPE:
                want = fixture["defaults"][dtype]
                for k in want:   # field by field: a difference names its field
                    assert m[k] == want[k], f"{dtype}: {k} differs from the recorded default manifest"
                assert m == want
            else:
                key = shape_key(dtype, cfg, hw, stacks)
                assert digest(m) == fixture["sha256"][key], f"the plan manifest of {key} changed"


def test_fixture_covers_every_configuration(fixture):
    assert set(fixture["defaults"]) == set(DTYPES)
    assert len(fixture["sha256"]) == len(DTYPES) * len(CONFIGS) * len(INPUTS) * len(STACKS) - len(DTYPES)


def test_set_option_refusals_keep_their_text(native_lib, fixture):
    got = option_errors(native_lib)   # (asserts DF3D_EINVAL for every out-of-range value)
    assert got == fixture["errors"]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deepfly3d_amd import _native

    fx = record(_native.load())
    with open(FIXTURE, "w") as f:   # one step / one parameter per line
        f.write(re.sub(r"\n {5,}|\n {4}(?=\])", " ", json.dumps(fx, indent=1, sort_keys=True)))
        f.write("\n")
    print(f"wrote {FIXTURE}: {len(fx['defaults'])} manifests, {len(fx['sha256'])} digests, {len(fx['errors'])} refusals")
