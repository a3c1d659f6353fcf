"""Bundle adjustment's host logic, pinned: the size of the LSMR work buffer (df3d_ba_lsmr_work_doubles) for a spread of problems and the
return code and text of every argument refusal that df3d_ba_lsmr_form, df3d_ba_trf_subspace and df3d_vec_dots decide before their first
HIP call must equal tests/golden/ba_host_pinned.json.  No device is needed: every call here returns before it touches one (the
"device" pointers are made-up addresses that are never dereferenced).

`python tests/test_ba_host_pinned.py` rewrites the fixture (after a deliberate change of the layout or of a refusal)."""
import ctypes
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_host_pinned.json")
# observations: 1; 1015 / 1016 / 1017 around one data-local range (1016 observations); the 1000-frame window's 106 k; 130 049 and 200 000,
# which need more data-local workgroups than the form has (128)
NOBS_NPTS = [(1, 1), (1015, 400), (1016, 1016), (1017, 509), (106000, 37000), (130049, 65025), (200000, 100000)]
NCAM = [1, 7, 8]
PTR = 0x1000        # a non-null "device pointer": the refusals are decided before anything reads it
LSMR_LAUNCHES = 2   # DF3D_LSMR_LAUNCHES of include/df3d_hip.h
NO_SUCH_FORM = 4


def problem(ncam=7, nobs=100, npts=40, arrays=PTR, **override):
    from deepfly3d_amd import _native

    fields = [f for f, _ in _native.BAProblem._fields_]
    assert fields[:3] == ["ncam", "nobs", "npts"]
    values = dict(ncam=ncam, nobs=nobs, npts=npts, **{f: arrays for f in fields[3:]})
    values.update(override)
    return _native.BAProblem(*[values[f] for f in fields])


def bad_problems():
    return [("null problem", None), ("ncam 0", problem(ncam=0)), ("ncam 9", problem(ncam=9)), ("empty problem: no observations", problem(nobs=0)),
            ("empty problem: no points", problem(npts=0)), ("null array", problem(cam_perm=None))]


def work_doubles(lib):
    out = {"null": lib.df3d_ba_lsmr_work_doubles(None)}
    for ncam in NCAM:
        for nobs, npts in NOBS_NPTS:
            out[f"{ncam}/{nobs}/{npts}"] = lib.df3d_ba_lsmr_work_doubles(ctypes.byref(problem(ncam, nobs, npts, arrays=None)))
    return out


def refusals(lib):
    """{entry point: {case: [return code, df3d_last_error]}}"""
    info = (ctypes.c_double * 8)()
    sub = (ctypes.c_double * 19)()

    def lsmr_form(p, form=LSMR_LAUNCHES, x=PTR):
        return lib.df3d_ba_lsmr_form(ctypes.byref(p) if p is not None else None, PTR, PTR, PTR, PTR, 0.37, 1e-6, 1e-6, 1e8, 16, x, PTR, info, None, form)

    def subspace(p, form=LSMR_LAUNCHES, delta=1.0, g_h=PTR):
        return lib.df3d_ba_trf_subspace(ctypes.byref(p) if p is not None else None, PTR, PTR, PTR, PTR, PTR, delta, g_h, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, sub,
                                        None, form)

    def dots(count, a):
        k = max(count, 1)
        n = (ctypes.c_size_t * k)(*[8] * k)
        out = (ctypes.c_double * k)()
        return lib.df3d_vec_dots(count, (ctypes.c_void_p * k)(*a[:k]), (ctypes.c_void_p * k)(*[PTR] * k), n, out, PTR, None)

    calls = {
        "df3d_ba_lsmr_form": [("unknown form", lambda: lsmr_form(problem(), form=NO_SUCH_FORM))]
        + [(name, lambda p=p: lsmr_form(p)) for name, p in bad_problems()]
        + [("null pointer", lambda: lsmr_form(problem(), x=None))],
        "df3d_ba_trf_subspace": [("unknown form", lambda: subspace(problem(), form=NO_SUCH_FORM))]
        + [(name, lambda p=p: subspace(p)) for name, p in bad_problems()]
        + [("null pointer", lambda: subspace(problem(), g_h=None)), ("Delta 0", lambda: subspace(problem(), delta=0.0)),
           ("Delta negative", lambda: subspace(problem(), delta=-1.0))],
        "df3d_vec_dots": [("count 0", lambda: dots(0, [PTR])), ("count 9", lambda: dots(9, [PTR] * 9)), ("null vector", lambda: dots(2, [PTR, None]))],
    }
    out = {}
    for entry, cases in calls.items():
        out[entry] = {}
        for name, call in cases:
            rc = call()
            assert rc != 0, f"{entry}: {name} was not refused"
            out[entry][name] = [rc, lib.df3d_last_error().decode()]
    return out


def record(lib):
    return {"work_doubles": work_doubles(lib), "refusals": refusals(lib)}


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_lsmr_work_buffer_size_is_unchanged(native_lib, fixture):
    got = work_doubles(native_lib)
    assert got["null"] == 0
    assert len(got) == 1 + len(NCAM) * len(NOBS_NPTS)
    for key, want in fixture["work_doubles"].items():
        assert got[key] == want, f"df3d_ba_lsmr_work_doubles({key}) changed"
    assert got == fixture["work_doubles"]


def test_argument_refusals_keep_their_code_and_text(native_lib, fixture):
    got = refusals(native_lib)
    for entry, cases in fixture["refusals"].items():
        for name, want in cases.items():
            assert got[entry][name] == want, f"{entry}: {name}"
    assert got == fixture["refusals"]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deepfly3d_amd import _native

    fx = record(_native.load())
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}: {len(fx['work_doubles'])} sizes, {sum(len(v) for v in fx['refusals'].values())} refusals")
