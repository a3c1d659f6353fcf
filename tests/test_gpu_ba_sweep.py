"""-m gpu sweep of the bundle-adjustment kernels (csrc/ba.hip, csrc/ba_lsmr.hip) over camera counts 1..8 and the edges of their layouts,
on the seeded problems of tests/ba_cases.py, against the float64 oracle (oracle/trf_lsmr.py, oracle/geometry.py).
tests/test_ba_cases_host.py checks on the CPU what each case reaches and that the oracle's decisions on it are robust; nothing here skips or
weakens at run time.  Every launch goes on ONE side stream, so the launch-based LSMR forms take their graph path and the graph cache sees
one problem after another; every output buffer is filled with NaN in front of the call under test."""
import ctypes
import math
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

import ba_cases as bc

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_first_launches = {}      # case -> (x, info) of its first LAUNCHES run, for the re-run behind the sweep
_graph_runs = []          # the cases whose LAUNCHES run replayed a recorded chunk, in order


@pytest.fixture(scope="module")
def stream(native_lib, cuda):
    return torch.cuda.Stream(device=cuda)


@pytest.fixture(autouse=True)
def _on_the_side_stream(stream):
    with torch.cuda.stream(stream):
        yield
    stream.synchronize()


def _nan(n, cuda):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=cuda)


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.fixture(scope="module", params=bc.CASE_NAMES)
def dev(request, native_lib, cuda, stream):
    """The case on the device: problem tables, the Jacobian blocks at its first evaluation point (df3d_ba_eval), the oracle's scaling and
    residual as the LSMR right-hand side."""
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, _Dev

    name = request.param
    case = bc.make_case(name)
    with torch.cuda.stream(stream):
        prob = BAProblemDevice(case["points2d_px"], case["intr"], cuda, min_views=case["min_views"])
        dv = _Dev(prob)
        Jc, Jp = _nan(12 * case["nobs"], cuda), _nan(6 * case["nobs"], cuda)
        if prob.nobs == case["nobs"] and prob.npts == case["npts"]:   # (test_tables reports a mismatch; no launch on wrong sizes)
            dv.eval(_up(bc.eval_points(name)[0], cuda), None, Jc, Jp)
        d, b = _up(bc.oracle_scale(name), cuda), _up(bc.oracle_blocks(name)[0], cuda)
        work = dv.new(dv.lib.df3d_ba_lsmr_work_doubles(ctypes.byref(prob.c)))
        stream.synchronize()
    return types.SimpleNamespace(name=name, case=case, prob=prob, dv=dv, Jc=Jc, Jp=Jp, d=d, b=b, work=work, out=_nan(case["n"], cuda))


def test_tables(dev):
    case, prob = dev.case, dev.prob
    assert (prob.ncam, prob.nobs, prob.npts, prob.m, prob.n) == (case["ncam"], case["nobs"], case["npts"], case["m"], case["n"])
    t = {k: v.cpu().numpy() for k, v in prob.t.items()}
    assert np.array_equal(t["cam_idx"], case["cam_idx"]) and np.array_equal(t["pt_idx"], case["pt_idx"])
    assert np.array_equal(t["obs_xy"], case["obs_xy"]) and np.array_equal(prob.slot, case["slot"])
    assert np.array_equal(t["pt_start"], np.concatenate([[0], np.cumsum(np.bincount(case["pt_idx"], minlength=case["npts"]))]))
    assert np.array_equal(t["cam_start"], np.concatenate([[0], np.cumsum(np.bincount(case["cam_idx"], minlength=case["ncam"]))]))
    assert np.array_equal(t["cam_perm"], np.argsort(case["cam_idx"], kind="stable"))


def test_eval(dev, cuda):
    case, prob, dv, nobs = dev.case, dev.prob, dev.dv, dev.case["nobs"]
    for which, x0 in enumerate(bc.eval_points(dev.name)):
        ref_r, ref_Jc, ref_Jp, _ = bc.oracle_blocks(dev.name, which)
        x = _up(x0, cuda)
        r, Jc, Jp = _nan(prob.m, cuda), _nan(12 * nobs, cuda), _nan(6 * nobs, cuda)
        dv.eval(x, r, Jc, Jp)
        got_Jc = Jc.cpu().numpy().reshape(2, 6, nobs).transpose(2, 0, 1)
        got_Jp = Jp.cpu().numpy().reshape(2, 3, nobs).transpose(2, 0, 1)
        e_r = np.abs(r.cpu().numpy() - ref_r).max()
        e_Jc = np.abs(got_Jc - ref_Jc).max() / np.abs(ref_Jc).max()
        e_Jp = np.abs(got_Jp - ref_Jp).max() / np.abs(ref_Jp).max()
        print("%s[%d] eval: r %.2e px (bar 1e-9)  Jc %.2e (1e-7)  Jp %.2e (1e-9)" % (dev.name, which, e_r, e_Jc, e_Jp))
        assert e_r < 1e-9 and e_Jc < 1e-7 and e_Jp < 1e-9      # (NaN -- an element no thread wrote -- fails every one of these)
        r2 = _nan(prob.m, cuda)
        dv.eval(x, r2, None, None)
        assert torch.equal(r, r2)                                 # the residual-only call: the same bits
        if dev.name == "small_rot" and which == 0:               # camera 0: r = 0, the first-order branch on both sides
            sel = case["cam_idx"] == 0
            e0 = np.abs(got_Jc[sel][:, :, :3] - ref_Jc[sel][:, :, :3]).max() / np.abs(ref_Jc[sel][:, :, :3]).max()
            print("small_rot camera 0 rotation columns: %.2e (bar 1e-12)" % e0)
            assert e0 < 1e-12


def test_matvec_rmatvec_colsq(dev, cuda):
    case, prob, dv, Jc, Jp = dev.case, dev.prob, dev.dv, dev.Jc, dev.Jp
    J = bc.oracle_blocks(dev.name)[3]
    rng = np.random.default_rng(0)
    v, u, d = rng.normal(size=prob.n), rng.normal(size=prob.m), rng.random(prob.n) + 0.5
    tv, tu, td = _up(v, cuda), _up(u, cuda), _up(d, cuda)
    y = dv.matvec(Jc, Jp, td, tv, _nan(prob.m, cuda))
    ref = J.matvec(d * v)
    e_mv = np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()
    w = dv.rmatvec(Jc, Jp, td, tu, _nan(prob.n, cuda))
    ref = d * J.rmatvec(u)
    e_rmv = np.abs(w.cpu().numpy() - ref).max() / np.abs(ref).max()
    w0 = dv.rmatvec(Jc, Jp, None, tu, _nan(prob.n, cuda))
    e_rmv0 = np.abs(w0.cpu().numpy() - J.rmatvec(u)).max() / np.abs(ref).max()
    cs = dv.colsq(Jc, Jp, _nan(prob.n, cuda))
    ref_cs = J.colsq()
    with np.errstate(invalid="ignore", divide="ignore"):
        e_cs = np.nanmax(np.where(ref_cs != 0, np.abs(cs.cpu().numpy() - ref_cs) / ref_cs, 0.0))
    print("%s: matvec %.2e (bar 1e-11)  rmatvec %.2e, without d %.2e (1e-11)  colsq %.2e (rtol 1e-12)" % (dev.name, e_mv, e_rmv, e_rmv0, e_cs))
    assert e_mv < 1e-11 and e_rmv < 1e-11 and e_rmv0 < 1e-11
    assert np.allclose(cs.cpu().numpy(), ref_cs, rtol=1e-12, atol=0)
    # a second call: the same bits
    assert torch.equal(y, dv.matvec(Jc, Jp, td, tv, _nan(prob.m, cuda)))
    assert torch.equal(w, dv.rmatvec(Jc, Jp, td, tu, _nan(prob.n, cuda)))
    assert torch.equal(w0, dv.rmatvec(Jc, Jp, None, tu, _nan(prob.n, cuda)))
    assert torch.equal(cs, dv.colsq(Jc, Jp, _nan(prob.n, cuda)))
    # a camera without observations: exactly 0 in its six entries, and scale 1 from the first update of the scaling
    from deepfly3d_amd import _native

    sci, sc = _nan(prob.n, cuda), _nan(prob.n, cuda)
    _native.check(dv.lib.df3d_ba_update_scale(cs.data_ptr(), sci.data_ptr(), sc.data_ptr(), prob.n, 1, dv.stream()))
    empty = np.flatnonzero(np.bincount(case["cam_idx"], minlength=case["ncam"]) == 0)
    assert dev.name != "edge_cams" or list(empty) == [0, 6]
    for c in empty:
        for vec in (w, w0, cs):
            assert bool((vec[6 * c : 6 * c + 6] == 0).all())
        assert bool((sc[6 * c : 6 * c + 6] == 1).all()) and bool((sci[6 * c : 6 * c + 6] == 1).all())
    assert np.allclose(sc.cpu().numpy(), bc.oracle_scale(dev.name), rtol=1e-12, atol=0)


def _run(dev, form, maxiter=0):
    """One LSMR run into the case's ONE output buffer (NaN in front): a copy of x, and info."""
    dev.out.fill_(float("nan"))
    info = dev.dv.lsmr(dev.Jc, dev.Jp, dev.d, dev.b, bc.DAMP, dev.out, dev.work, maxiter=maxiter, form=form)
    torch.cuda.current_stream().synchronize()
    return dev.out.clone(), info


def _check_against_oracle(what, x, info, ref):
    assert (int(info[0]), int(info[1])) == (ref[1], ref[2]), (what, info[:2], ref[1:3])   # same stop reason, same iteration count
    err = np.abs(x.cpu().numpy() - ref[0]).max() / np.abs(ref[0]).max()
    assert err < 1e-6, (what, err)
    return err


def _forms(name):
    from deepfly3d_amd import _native

    forms = [("eleven", _native.LSMR_ELEVEN), ("launches", _native.LSMR_LAUNCHES), ("barriers", _native.LSMR_BARRIERS), ("local", _native.LSMR_LOCAL)]
    return forms[1:] if name in ("max_fit", "over_fit") else forms   # (the eleven-kernel form is left out of the two large cases to keep them short)


def test_lsmr_forms(dev, monkeypatch):
    """Every form on the same buffers, one after the other: the launch-based forms look their chunk up in the graph cache under the same
    pointers and dimensions.  `tiny`, `eight_1024` and `mixed` also run capped, `tiny` and `mixed` the persistent form on small grids."""
    ref = bc.oracle_lsmr(dev.name)
    got, errs = {}, {}
    for label, form in _forms(dev.name):
        got[label] = _run(dev, form)
        errs[label] = _check_against_oracle((dev.name, label), *got[label], ref)
    print("%s: lsmr (istop, itn) = %s; x vs oracle (bar 1e-6): %s" % (dev.name, ref[1:3], "  ".join("%s %.2e" % kv for kv in errs.items())))
    xl, il = got["launches"]
    _first_launches.setdefault(dev.name, (xl, il))
    if min(dev.case["m"], dev.case["n"]) >= 16:
        _graph_runs.append(dev.name)
    for label in ("eleven", "barriers"):
        if label in got:
            assert torch.equal(got[label][0], xl) and got[label][1][:7] == il[:7], label   # identical bits
            assert got[label][1][7] == 0
    assert il[7] == 0
    x, info = got["local"]
    if dev.name == "over_fit":
        assert info[7] == 2, "129 workgroups: the data-local form must refuse"
        assert torch.equal(x, xl) and info[:7] == il[:7]                                    # ... and return the launch-based form's run
    else:
        assert info[7] == 0, "the data-local form fell back (1: its workgroups were not co-resident, 2: it refused the layout): %r" % (info[7],)
    x2, info2 = _run(dev, _forms(dev.name)[-1][1])
    assert torch.equal(x, x2) and info == info2                                              # a second data-local run: the same bits
    if dev.name in ("tiny", "eight_1024", "mixed"):
        _capped_runs(dev)
    if dev.name in ("tiny", "mixed"):
        _small_grid_runs(dev, monkeypatch, got["launches"])


def _capped_runs(dev):
    """maxiter 1, 15, 16, 17: the direct path, exactly one replayed chunk, a chunk plus the flush -- against the oracle at the same maxiter."""
    for maxiter in sorted({min(k, dev.case["m"], dev.case["n"]) for k in (1, 15, 16, 17)}):
        ref = bc.oracle_lsmr(dev.name, maxiter)
        got = {}
        for label, form in _forms(dev.name):
            got[label] = _run(dev, form, maxiter)
            err = _check_against_oracle((dev.name, label, maxiter), *got[label], ref)
            print("%s maxiter %d %s: (istop, itn) = %s, x vs oracle %.2e (bar 1e-6)" % (dev.name, maxiter, label, ref[1:3], err))
        for label in ("eleven", "barriers"):
            assert torch.equal(got[label][0], got["launches"][0]) and got[label][1][:7] == got["launches"][1][:7], (label, maxiter)
        assert all(g[1][7] == 0 for g in got.values())


def _small_grid_runs(dev, monkeypatch, launches):
    """The persistent form with 1 workgroup (no grid barrier at all) and 3 (divides no phase's virtual grid): the launch-based form's bits."""
    from deepfly3d_amd import _native

    for grid in ("1", "3"):
        monkeypatch.setenv("DF3D_LSMR_GRID", grid)
        xb, ib = _run(dev, _native.LSMR_BARRIERS)
        assert torch.equal(xb, launches[0]) and ib[:7] == launches[1][:7] and ib[7] == 0, grid
    monkeypatch.delenv("DF3D_LSMR_GRID")


def test_lsmr_launches_again_behind_the_sweep(native_lib, cuda, stream):
    """The first case, and the first case whose run replays a recorded chunk, once more: the graph cache has been replaced many times since."""
    from deepfly3d_amd import _native
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, _Dev

    assert list(_first_launches)[: 2] == list(bc.CASE_NAMES[:2]) and len(_first_launches) == len(bc.CASE_NAMES), "this test runs behind the sweep"
    assert _graph_runs[0] == bc.CASE_NAMES[1] and len(_graph_runs) >= 10
    for name in bc.CASE_NAMES[:2]:
        case = bc.make_case(name)
        prob = BAProblemDevice(case["points2d_px"], case["intr"], cuda, min_views=case["min_views"])
        dv = _Dev(prob)
        Jc, Jp = _nan(12 * case["nobs"], cuda), _nan(6 * case["nobs"], cuda)
        dv.eval(_up(case["x0"], cuda), None, Jc, Jp)
        d, b = _up(bc.oracle_scale(name), cuda), _up(bc.oracle_blocks(name)[0], cuda)
        work = dv.new(dv.lib.df3d_ba_lsmr_work_doubles(ctypes.byref(prob.c)))
        again = types.SimpleNamespace(dv=dv, Jc=Jc, Jp=Jp, d=d, b=b, work=work, out=_nan(case["n"], cuda))
        x, info = _run(again, _native.LSMR_LAUNCHES)
        assert torch.equal(x, _first_launches[name][0]) and info == _first_launches[name][1], name


@pytest.mark.parametrize("name", bc.SOLVE_CASES)
def test_whole_solve(native_lib, cuda, monkeypatch, name):
    from deepfly3d_amd.bundle_adjust import bundle_adjust

    case, want = bc.make_case(name), bc.SOLVES[name]
    Ro, to, res = bc.oracle_solve(name)
    assert (res["nfev"], res["status"], res["lsmr_iters"]) == (want["nfev"], want["status"], want["lsmr_iters"])
    bar_R, bar_t = max(100 * want["spread_R"], 1e-12), max(100 * want["spread_t"], 1e-12)
    for form in ("0", "2"):
        monkeypatch.setenv("DF3D_LSMR_KERNELS", form)
        got = []
        for host in ("1", "0"):
            monkeypatch.setenv("DF3D_TRF_HOST_SCALARS", host)
            R, t, info = bundle_adjust(case["points2d_px"], case["R_init"], case["tvec_init"], case["intr"], device=cuda, return_info=True)
            got.append((R, t, info["cost"], info["nfev"], info["njev"], info["status"], info["lsmr_iters"], info["optimality"], info["lsmr_fallbacks"]))
        R, t = got[0][:2]
        print("%s form %s: nfev %d status %d lsmr %s  |R - oracle| %.2e (bar %.1e)  |t - oracle| %.2e (bar %.1e)"
              % (name, form, got[0][3], got[0][5], got[0][6], np.abs(R - Ro).max(), bar_R, np.abs(t - to).max(), bar_t))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2:] == got[1][2:], form   # bit for bit
        assert (got[0][3], got[0][5], got[0][6]) == (res["nfev"], res["status"], res["lsmr_iters"])
        assert got[0][8] == 0
        assert np.abs(R - Ro).max() <= bar_R and np.abs(t - to).max() <= bar_t


def test_trf_step_counts_the_refusal_of_over_fit(native_lib, cuda, monkeypatch):
    """One outer iteration of the device-scalar driver on 129 workgroups' worth of observations: df3d_ba_trf_subspace takes the launch-based
    form, says so, and lands on that form's bits."""
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, solve_trf

    case = bc.make_case("over_fit")
    prob = BAProblemDevice(case["points2d_px"], case["intr"], cuda)
    x0 = _up(case["x0"], cuda)
    monkeypatch.delenv("DF3D_LSMR_KERNELS", raising=False)
    monkeypatch.delenv("DF3D_TRF_HOST_SCALARS", raising=False)
    a = solve_trf(prob, x0, max_nfev=2)
    xa = a["x"].clone()
    monkeypatch.setenv("DF3D_LSMR_KERNELS", "2")
    b = solve_trf(prob, x0, max_nfev=2)
    assert a["nfev"] == b["nfev"] == 2 and len(a["lsmr_iters"]) == 1
    assert a["lsmr_fallbacks"] == 1 and b["lsmr_fallbacks"] == 0
    assert a["lsmr_iters"] == b["lsmr_iters"] and a["cost"] == b["cost"] and torch.equal(xa, b["x"])
    assert bool(torch.isfinite(xa).all()) and not torch.equal(xa, x0)


# ---- the generic reductions: one element per thread up to RED_BLOCKS * 256 = 65 536 elements, a grid-stride loop above
LENGTHS = (1, 255, 256, 257, 65535, 65536, 65537, 200003)


@pytest.fixture(scope="module")
def vec(native_lib, cuda, stream):
    from deepfly3d_amd.bundle_adjust import _Dev

    rng = np.random.default_rng(7)
    host = {n: (rng.normal(size=n), rng.normal(size=n)) for n in LENGTHS}
    with torch.cuda.stream(stream):
        devv = {n: (_up(a, cuda), _up(b, cuda)) for n, (a, b) in host.items()}
        dv = _Dev(types.SimpleNamespace(device=cuda))
    return types.SimpleNamespace(host=host, dev=devv, dv=dv)


def test_vec_dot_and_dots(vec):
    singles = []
    for n in LENGTHS:
        (a, b), (ta, tb) = vec.host[n], vec.dev[n]
        got = vec.dv.dot(ta, tb)
        bound = 8 * EPS * math.fsum(np.abs(a * b))
        err = abs(got - math.fsum(a * b))
        print("dot n=%d: |err| %.2e (bound %.2e)" % (n, err, bound))
        assert err <= bound
        assert vec.dv.dot(ta, tb) == got                          # a second call: the same bits
        singles.append(got)
    assert vec.dv.dots(*[vec.dev[n] for n in LENGTHS]) == singles  # eight products of mixed lengths in one call: each one's bits
    assert vec.dv.dots(*[vec.dev[n] for n in reversed(LENGTHS)]) == singles[::-1]


def test_vec_pairnorm_sum(vec, cuda):
    from deepfly3d_amd import _native

    dv = vec.dv
    for n in LENGTHS:
        r = np.stack(vec.host[n], axis=1).ravel()   # n (x, y) pairs
        tr = _up(r, cuda)
        got = []
        for _ in range(2):
            _native.check(dv.lib.df3d_vec_pairnorm_sum(tr.data_ptr(), n, ctypes.byref(dv._res), dv.scratch.data_ptr(), dv.stream()))
            got.append(dv._res.value)
        norms = np.sqrt(r[0::2] ** 2 + r[1::2] ** 2)
        err, bound = abs(got[0] - math.fsum(norms)), 8 * EPS * math.fsum(norms)
        print("pairnorm_sum n=%d: |err| %.2e (bound %.2e)" % (n, err, bound))
        assert err <= bound and got[0] == got[1]


def test_vec_absmax(vec, cuda):
    for n in LENGTHS:
        a = vec.host[n][0].copy()
        a[-1] = -(np.abs(a).max() + 1.0)                          # the maximum in the last element, negative
        assert vec.dv.absmax(_up(a, cuda)) == np.abs(a).max() == -a[-1]
        assert vec.dv.absmax(vec.dev[n][0]) == np.abs(vec.host[n][0]).max()
        z = vec.dv.absmax(_up(np.full(n, -0.0), cuda))
        assert z == 0.0 and math.copysign(1.0, z) == 1.0


def _one_fma_values(a, x, b, y):
    """a x + b y with ONE of the two products fused into the addition (a single rounding of  fl(a x) + b y,  or of  a x + fl(b y)), exactly."""
    f = Fraction
    return float(f(float(a * x)) + f(b) * f(y)), float(f(a) * f(x) + f(float(b * y)))


def test_vec_axpby_and_mul(vec, cuda):
    """out = a x + b y: csrc/ba.hip is compiled with floating-point contraction, which lets the compiler fuse one of the two products into
    the addition (v = a x; v += b y  becomes  fma(b, y, fl(a x)), or the mirror image -- the language leaves the choice to it).  Accepted per
    element: numpy's value (both products rounded, then the sum), or the value with exactly one product left unrounded -- at least as
    close to the exact result, and the only freedom contraction gives a two-product sum.  Nothing else (a wrong index, a stale element, a
    different coefficient) fits either.  a x alone and x y have one rounding: numpy's bits."""
    dv, a, b = vec.dv, 1.7, -0.3
    for n in LENGTHS:
        (x, y), (tx, ty) = vec.host[n], vec.dev[n]
        got = dv.axpby(a, tx, b, ty, _nan(n, cuda)).cpu().numpy()
        inplace = tx.clone()
        dv.axpby(a, inplace, b, ty, inplace)
        assert np.array_equal(inplace.cpu().numpy(), got)         # in place over x: the same values
        inplace = ty.clone()
        dv.axpby(a, tx, b, inplace, inplace)
        assert np.array_equal(inplace.cpu().numpy(), got)         # in place over y
        ref = a * x + b * y
        off = np.flatnonzero(got != ref)
        for i in off[:: max(1, off.size // 2000)]:                # (exact rational arithmetic: every differing element up to 2 000, a comb above)
            assert got[i] in _one_fma_values(a, x[i], b, y[i]), (n, i, got[i], ref[i])
        assert np.abs(got - ref).max() <= 2 * EPS * (np.abs(a * x) + np.abs(b * y)).max()   # (all of them: within one rounding of numpy's)
        print("axpby n=%d: %d of %d elements differ from numpy's double rounding by a fused multiply-add" % (n, off.size, n))
        assert np.array_equal(dv.axpby(a, tx, 0.0, None, _nan(n, cuda)).cpu().numpy(), a * x)
        assert np.array_equal(dv.mul(tx, ty, _nan(n, cuda)).cpu().numpy(), x * y)


def test_update_scale(vec, cuda):
    from deepfly3d_amd import _native

    dv = vec.dv
    rng = np.random.default_rng(8)
    for n in LENGTHS:
        s1, s2 = rng.integers(0, 1000, size=n) / 8.0, rng.integers(0, 1000, size=n) / 8.0   # (their squares and square roots are exact)
        s1[-1] = 0.0
        sci, sc = _nan(n, cuda), _nan(n, cuda)
        _native.check(dv.lib.df3d_ba_update_scale(_up(s1 * s1, cuda).data_ptr(), sci.data_ptr(), sc.data_ptr(), n, 1, dv.stream()))
        want = np.where(s1 == 0, 1.0, s1)                         # first: zeros -> 1
        assert np.array_equal(sci.cpu().numpy(), want) and np.array_equal(sc.cpu().numpy(), 1.0 / want)
        _native.check(dv.lib.df3d_ba_update_scale(_up(s2 * s2, cuda).data_ptr(), sci.data_ptr(), sc.data_ptr(), n, 0, dv.stream()))
        want = np.maximum(s2, want)                               # later: the running maximum (a zero does not become 1 any more)
        assert np.array_equal(sci.cpu().numpy(), want) and np.array_equal(sc.cpu().numpy(), 1.0 / want)
