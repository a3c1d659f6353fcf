"""Bundle adjustment on the device, pinned bit for bit: SHA-256 digests of what every explicitly chosen LSMR form and both trust-region
drivers compute on the reference's 15-frame sample problem, and of the data-local form's fallback on a single-view problem, must equal
tests/golden/ba_gpu_digests.json.  Every sum on these paths has a fixed order, so a run reproduces itself; a host-side change that moves
one HIP call, one buffer or one scalar shows here.

Everything runs once, in one process, on a side stream (the chunks of the launch-based forms are replayed from a HIP graph there).
`python tests/test_gpu_ba_pinned.py [OUT.json]` rewrites the fixture (or writes OUT.json) on a GPU."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "ba_gpu_digests.json")
FORMS = {"ELEVEN": 11, "LAUNCHES": 2, "BARRIERS": 1, "LOCAL": 3}   # DF3D_LSMR_* of include/df3d_hip.h
# one whole chunk of 16 iterations; a chunk and one iteration; two chunks and one; convergence (several chunks, a partial one; < 200 iterations)
MAXITER = (16, 17, 33, 1000)
TRF_FORMS = {"AUTO": 0, "LAUNCHES": 2}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def lsmr_digest(x, info):
    return {"x": sha(x.cpu().numpy()), "info": sha(np.array(info)), "istop": info[0], "itn": info[1], "fallback": info[7]}


def linearised(ba, _native, prob, x0):
    """f, J and the column scaling at x0 (tests/perf/lsmr_dump.py's set-up)"""
    dv = ba._Dev(prob)
    m, n, nobs = prob.m, prob.n, prob.nobs
    f, Jc, Jp, sc, sci, tmp = dv.new(m), dv.new(12 * nobs), dv.new(6 * nobs), dv.new(n), dv.new(n), dv.new(n)
    dv.eval(x0, f, Jc, Jp)
    dv.colsq(Jc, Jp, tmp)
    _native.check(dv.lib.df3d_ba_update_scale(tmp.data_ptr(), sci.data_ptr(), sc.data_ptr(), n, 1, dv.stream()))
    return dv, f, Jc, Jp, sc


def lsmr_runs(ba, prob, lin, forms, maxiters):
    """Every form on buffers of its own, all kept alive to the end: the recorded chunk is looked up by its buffers, not by its form."""
    import torch

    dv, f, Jc, Jp, sc = lin
    out, keep = {}, []
    for name in forms:
        work = dv.new(dv.lib.df3d_ba_lsmr_work_doubles(ctypes.byref(prob.c)))
        xs = dv.new(prob.n)
        keep.append((work, xs))
        for mi in maxiters:
            info = dv.lsmr(Jc, Jp, sc, f, 0.37, xs, work, maxiter=mi, form=FORMS[name])
            torch.cuda.synchronize()
            out[f"{name}/{mi}"] = lsmr_digest(xs, info)
    return out, keep


def compute(dev):
    import torch

    from deepfly3d_amd import _native, ops
    from deepfly3d_amd import bundle_adjust as ba
    from deepfly3d_amd.config import load_calibration

    g = np.load(os.path.join(GOLDEN, "golden_2d.npz"))
    cal = load_calibration()
    c = {k: np.stack([cal[i][k] for i in range(7)]) for k in ("R", "tvec", "intr")}
    px = g["points2d"] * np.array([480.0, 960.0])
    cams = np.concatenate([np.stack([ba._rotvec_from_matrix(c["R"][k]) for k in range(7)]), c["tvec"]], axis=1).ravel()
    out = {}
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        # the reference's sample problem, 15 frames
        prob = ba.BAProblemDevice(px, c["intr"], dev)
        P = np.einsum("cij,cjk->cik", c["intr"], np.concatenate([c["R"], c["tvec"][..., None]], axis=-1))
        X0 = ops.triangulate(P, torch.from_numpy(np.ascontiguousarray(px)).to(dev))
        x0 = torch.cat([torch.from_numpy(cams).to(dev), X0.reshape(-1, 3)[prob.ok_dev].reshape(-1)])
        out["lsmr"], keep = lsmr_runs(ba, prob, linearised(ba, _native, prob, x0), list(FORMS), MAXITER)
        out["solve_trf"] = {}
        for device_scalars in (True, False):
            for name, form in TRF_FORMS.items():
                res = ba.solve_trf(prob, x0, lsmr_form=form, device_scalars=device_scalars)
                cam = res["x"][:42].cpu().numpy().reshape(7, 6)
                R = np.stack([ba._matrix_from_rotvec(cam[k, :3]) for k in range(7)])
                out["solve_trf"][f"device_scalars={device_scalars}/{name}"] = {
                    "Rt": sha(R, cam[:, 3:]), "x": sha(res["x"].cpu().numpy()),
                    "result": [res["cost"], res["nfev"], res["njev"], res["status"], res["lsmr_iters"], res["optimality"], res["lsmr_fallbacks"]]}
        # single-view points (tests/test_gpu_ba.py: test_data_local_lsmr_refuses_problems_outside_its_layout_and_falls_back): the data-local
        # form does not fit, LOCAL falls back to LAUNCHES
        px1 = np.tile(px, (1, 4, 1, 1))
        seen = px1[..., 0] != 0
        first_cam = np.arange(px1.shape[0])[:, None, None] == np.argmax(seen, axis=0)[None]
        px1 = np.where((seen & first_cam)[..., None], px1, 0.0)
        prob1 = ba.BAProblemDevice(px1, c["intr"], dev, min_views=1)
        rng = np.random.default_rng(1)
        x1 = torch.from_numpy(np.concatenate([cams, rng.normal(0, 1, size=3 * prob1.npts) + np.tile([0.0, 0.0, 100.0], prob1.npts)])).to(dev)
        out["single_view"], keep1 = lsmr_runs(ba, prob1, linearised(ba, _native, prob1, x1), ["LAUNCHES", "LOCAL"], (40,))
    torch.cuda.synchronize()
    del keep, keep1
    return out


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(native_lib, cuda):
    return compute(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_lsmr_form_digests_are_unchanged(got, fixture, form):
    for mi in MAXITER:
        key = f"{form}/{mi}"
        print(key, got["lsmr"][key])
        assert got["lsmr"][key]["fallback"] == 0, f"{key} ran through its fallback"
        assert got["lsmr"][key] == fixture["lsmr"][key], f"LSMR {key} changed"


@pytest.mark.gpu
def test_solve_trf_digests_are_unchanged(got, fixture):
    assert set(got["solve_trf"]) == set(fixture["solve_trf"]) and len(got["solve_trf"]) == 4
    for key, want in fixture["solve_trf"].items():
        print(key, got["solve_trf"][key])
        assert got["solve_trf"][key] == want, f"solve_trf {key} changed"


@pytest.mark.gpu
def test_single_view_fallback_digests_are_unchanged(got, fixture):
    print(got["single_view"])
    assert got["single_view"]["LOCAL/40"]["fallback"] == 2 and fixture["single_view"]["LOCAL/40"]["fallback"] == 2   # (does not fit)
    assert got["single_view"]["LAUNCHES/40"]["fallback"] == 0
    assert got["single_view"] == fixture["single_view"]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    fx = compute(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(fx['lsmr'])} + {len(fx['single_view'])} LSMR runs, {len(fx['solve_trf'])} adjustments")
