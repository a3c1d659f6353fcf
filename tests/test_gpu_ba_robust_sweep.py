"""-m gpu sweep of the robust-loss bundle adjustment's kernels ("Sweep"): ba_eval_robust_kernel on the residual dial
of tests/ba_robust_dial.py -- every residual a chosen number, so df3d_robust::row() is probed in its cancellation zones, on both sides of
the clamp and at huber's branch point --, all eight combinations of its optional outputs, robust_cost_kernel over the vector lengths of
tests/test_gpu_ba_sweep.py (its grid-stride loop's second lap), one rho at a time against 50-digit arithmetic, and residuals that are
not finite.  tests/test_ba_robust_dial_host.py checks on the CPU every condition relied on here.  The whole solves under huber, cauchy and
arctan are cases of tests/test_gpu_ba_robust.py::test_whole_solve.  Every launch goes on one side stream; every output buffer is filled
with NaN in front of the call under test."""
import math
import types

import numpy as np
import pytest
import torch

import ba_robust_dial as dial
import ba_robust_oracle as bro
from test_gpu_ba_sweep import LENGTHS

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ULP = 64 * EPS          # the bar of tests/test_gpu_ba_robust.py for scaled f, weights and scaled J
RHO_ULP = 4             # one rho against 50 digits, in EPS: 4 x the larger of what numpy (0.76) and the device (0.93) measure on the probe values,
                        # rounded up -- the device math library's documented bounds are not at hand ("Sweep")
SQRT_EPS = 2.0**-26     # a clamped row's s, to the bit
GUARD, GUARD_VALUE = 16, -7.25
LAP = 65536             # RED_BLOCKS * 256 lanes: robust_cost_kernel's grid-stride loop takes a second lap above this


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


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _rel(got, want):
    """max |got - want| / |want| where want != 0; elements where want == 0 must be 0."""
    zero = want == 0
    assert np.array_equal(got[zero], want[zero])
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if (~zero).any() else 0.0


def _device_problem(px, intr, cuda):
    from deepfly3d_amd.bundle_adjust import BAProblemDevice, _Dev

    prob = BAProblemDevice(px, intr, cuda, min_views=2)
    return prob, _Dev(prob)


@pytest.fixture(scope="module", params=dial.F_SCALES)
def dials(request, native_lib, cuda, stream):
    """The dial's problems of one f_scale on the device."""
    C = request.param
    out = []
    with torch.cuda.stream(stream):
        for p in dial.problems(C):
            prob, dv = _device_problem(p["px"], p["intr"], cuda)
            assert (prob.nobs, prob.npts, prob.m) == (p["nobs"], p["npts"], 2 * p["nobs"])
            out.append(types.SimpleNamespace(p=p, prob=prob, dv=dv, x=_up(p["x"], cuda)))
        stream.synchronize()
    return types.SimpleNamespace(C=C, problems=out)


def _run(d, code, C, cuda):
    """One full evaluation of a dial problem: f_true, scaled f, w, and s as the four planes that hold it (Jp (0, 0) / (1, 1) and the Jc
    translation planes (0, 3) / (1, 4), interleaved into residual order), plus the raw Jc, Jp."""
    nobs, m = d.prob.nobs, d.prob.m
    ft, f, w, Jc, Jp = _nan(m, cuda), _nan(m, cuda), _nan(m, cuda), _nan(12 * nobs, cuda), _nan(6 * nobs, cuda)
    d.dv.eval_robust(d.x, code, C, f, Jc, Jp, f_true=ft, w=w)
    jc, jp = Jc.cpu().numpy().reshape(2, 6, nobs), Jp.cpu().numpy().reshape(2, 3, nobs)
    s_p, s_c = np.stack([jp[0, 0], jp[1, 1]], axis=1).ravel(), np.stack([jc[0, 3], jc[1, 4]], axis=1).ravel()
    return types.SimpleNamespace(f_true=ft.cpu().numpy(), f=f.cpu().numpy(), w=w.cpu().numpy(), s=s_p, s_c=s_c, Jc=Jc, Jp=Jp, jc=jc, jp=jp, tf=f, tw=w, tft=ft)


def _assert_the_dial_is_right(got, p):
    ok = np.array_equal(got.f_true, p["planted"]) and np.array_equal(np.signbit(got.f_true), np.signbit(p["planted"]))
    assert ok, "THE DIAL IS WRONG, not the kernel: the unscaled residuals are not the planted values bit for bit (nobs %d)" % p["nobs"]


def test_the_table_on_the_dial(dials, cuda):
    """w, s and the scaled f within 64 ulp of the oracle evaluated on the device's own f_true, on every dial row: the cancellation
    zones 1 - z ~ 0 and 1 - 3 z^2 ~ 0, the ladders through (EPS, 1e-6), z = 1 and its neighbours, +0, z that underflows, t * t that
    overflows.  The bar holds in the cancellation zones because 1 - z is exact for z in [1/2, 2] and so is 1 - fl(3 z^2): two
    computations that agree on z to the bit differ only in the quotient's and the root's roundings, one that does not agree on z (a
    product fused past rounded()) is off by far more.  The clamped set is exactly the oracle's."""
    from deepfly3d_amd import _native

    C = dials.C
    for loss in bro.LOSSES:
        code = _native.BA_LOSSES.index(loss)
        worst, differ, rows, n_clamped = dict(w=0.0, s=0.0, f=0.0), 0, 0, 0
        for d in dials.problems:
            p = d.p
            got = _run(d, code, C, cuda)
            _assert_the_dial_is_right(got, p)
            assert np.array_equal(got.s.view(np.int64), got.s_c.view(np.int64))                 # the Jp planes and the Jc planes: one s
            assert not np.isnan(got.jc).any() and not np.isnan(got.jp).any()                    # every plane written
            assert (got.jp[0, 1] == 0).all() and (got.jp[1, 0] == 0).all() and (got.jc[0, 4] == 0).all() and (got.jc[1, 3] == 0).all()
            z, want_w, want_s, want_f, clamped = dial.oracle_rows(loss, got.f_true, C)
            assert np.isfinite(want_w).all() and np.isfinite(want_s).all() and np.isfinite(want_f).all()
            e = dict(w=_rel(got.w, want_w), s=_rel(got.s, want_s), f=_rel(got.f, want_f))
            assert max(e.values()) <= ULP, (loss, C, p["nobs"], e)
            got_clamped = got.s == SQRT_EPS
            wrong = np.flatnonzero(got_clamped != clamped)
            assert wrong.size == 0, (loss, C, p["nobs"], [(float(got.f_true[i]), float(z[i]), bool(clamped[i])) for i in wrong[:8]])
            for k in worst:
                worst[k] = max(worst[k], e[k] / ULP)
            differ += int((got.w != want_w).sum() + (got.s != want_s).sum() + (got.f != want_f).sum())
            rows += z.size
            n_clamped += int(clamped.sum())
        print("dial %s C=%g: worst ratio to the 64 ulp bar: %s;  %d of 3 x %d values differ from the oracle's bits (%s);  %d rows clamped"
              % (loss, C, "  ".join("%s %.3f" % kv for kv in worst.items()), differ, rows, "bit for bit" if differ == 0 else "NOT bit for bit", n_clamped))


def test_optional_outputs_all_eight_combinations(dials, cuda):
    """f_true, w and Jc / Jp (together) are three independent switches: every output that is given is bit-equal to the all-given run,
    and the 16 guard doubles behind every buffer stay untouched.  On the two-block dial problem (258 observations), every loss."""
    from deepfly3d_amd import _native

    C = dials.C
    d = dials.problems[-1]
    nobs, m = d.prob.nobs, d.prob.m
    assert nobs == 258

    def buf(n):
        b = _nan(n + GUARD, cuda)
        b[n:] = GUARD_VALUE
        return b

    for loss in bro.LOSSES:
        code = _native.BA_LOSSES.index(loss)
        full = _run(d, code, C, cuda)
        _assert_the_dial_is_right(full, d.p)
        ref = dict(f=_bits(full.tf), ft=_bits(full.tft), w=_bits(full.tw), Jc=_bits(full.Jc), Jp=_bits(full.Jp))
        for combo in range(8):
            want_ft, want_w, want_J = bool(combo & 1), bool(combo & 2), bool(combo & 4)
            b = dict(f=buf(m), ft=buf(m) if want_ft else None, w=buf(m) if want_w else None, Jc=buf(12 * nobs) if want_J else None,
                     Jp=buf(6 * nobs) if want_J else None)
            view = {k: (None if v is None else v[: v.numel() - GUARD]) for k, v in b.items()}
            assert all(v is None or v.data_ptr() == b[k].data_ptr() for k, v in view.items())
            d.dv.eval_robust(d.x, code, C, view["f"], view["Jc"], view["Jp"], f_true=view["ft"], w=view["w"])
            for k, v in b.items():
                if v is None:
                    continue
                host = v.cpu().numpy()
                assert (host[-GUARD:] == GUARD_VALUE).all(), (loss, combo, k, "a guard double was written")
                assert np.array_equal(host[:-GUARD].view(np.int64), ref[k]), (loss, combo, k)


@pytest.fixture(scope="module")
def long_vectors(native_lib, cuda, stream):
    """Seeded standard-normal vectors of every length (times C: z = N(0, 1)^2 straddles 1); the single-element length gets one value on
    either side."""
    from deepfly3d_amd.bundle_adjust import _Dev

    assert LENGTHS == (1, 255, 256, 257, 65535, 65536, 65537, 200003) and LENGTHS[-2] > LAP >= LENGTHS[-3]
    rng = np.random.default_rng(11)
    host = {n: ([rng.normal(size=n)] if n > 1 else [np.array([0.6]), np.array([1.7])]) for n in LENGTHS}
    with torch.cuda.stream(stream):
        dv = _Dev(types.SimpleNamespace(device=cuda))
    return types.SimpleNamespace(host=host, dv=dv)


@pytest.mark.parametrize("C", (0.5, 5.0))
def test_long_costs(long_vectors, cuda, C):
    """df3d_ba_robust_cost within 24 EPS fsum(terms) of 1/2 C^2 fsum(rho) of the oracle's element-wise rho -- 8 for the summation, the
    bound tests/test_gpu_ba_sweep.py uses for dot, 16 for one rho -- from one element to 200 003: one block, a partial block, the whole
    grid, and the grid-stride loop's second lap (above 65 536).  A second call returns the same bits."""
    from deepfly3d_amd import _native

    dv = long_vectors.dv
    worst = {}
    for n in LENGTHS:
        vecs = [C * u for u in long_vectors.host[n]]
        z_all = np.concatenate([(v / C) ** 2 for v in vecs])
        assert (z_all < 1).any() and (z_all > 1).any(), "the residuals have to lie on both sides of z = 1"
        for v in vecs:
            tv = _up(v, cuda)
            for loss in bro.LOSSES:
                terms = 0.5 * C * C * bro.rho(loss, (v / C) ** 2)
                assert (terms >= 0).all()
                want = 0.5 * C * C * math.fsum(bro.rho(loss, (v / C) ** 2))
                bound = 24 * EPS * math.fsum(terms)
                got = dv.robust_cost(tv, _native.BA_LOSSES.index(loss), C)
                assert abs(got - want) <= bound, (loss, C, n, got, want, abs(got - want) / bound)
                assert dv.robust_cost(tv, _native.BA_LOSSES.index(loss), C) == got
                worst[loss] = max(worst.get(loss, 0.0), abs(got - want) / bound)
    print("long costs C=%g: worst ratio to the 24 EPS fsum(terms) bound over %s: %s" % (C, LENGTHS, "  ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("C", dial.F_SCALES)
def test_one_rho_at_a_time(long_vectors, cuda, C):
    """m = 1: the cost of one residual is 1/2 C^2 rho(z), compared with 50-digit arithmetic at the float64 z on the dial's probe values
    (z = 1 and its neighbours, arctan's zero, the ladders' ends, z = 0 from +0, -0 and an underflow, z up to 2^500).  huber, cauchy,
    arctan and linear relative; soft_l1 absolute against sqrt(1 + z), because 2 (sqrt(1 + z) - 1) cancels for small z, in scipy as
    here.  numpy's own figure is printed beside the device's."""
    import mpmath as mp

    from deepfly3d_amd import _native

    dv = long_vectors.dv
    probe = dial.rho_probe(C)
    z = (probe / C) ** 2
    tv = _up(probe, cuda)
    half_c2 = 0.5 * C * C
    for loss in bro.LOSSES:
        code = _native.BA_LOSSES.index(loss)
        worst_dev = worst_np = 0.0
        for i in range(probe.size):
            got = dv.robust_cost(tv[i : i + 1], code, C)
            ref = dial.mp_rho(loss, z[i])
            host = float(bro.rho(loss, z[i]))
            if ref == 0:
                assert got == 0 and host == 0, (loss, C, probe[i])
                continue
            with mp.workdps(50):
                scale = mp.sqrt(1 + mp.mpf(float(z[i]))) if loss == "soft_l1" else ref
                e_dev = float(abs(mp.mpf(got) / mp.mpf(half_c2) - ref) / scale) / EPS
                e_np = float(abs(mp.mpf(host) - ref) / scale) / EPS
            assert e_dev <= RHO_ULP, (loss, C, float(probe[i]), float(z[i]), got, e_dev)
            worst_dev, worst_np = max(worst_dev, e_dev), max(worst_np, e_np)
        print("one rho %s C=%g: against 50 digits, in EPS: device %.2f, numpy %.2f (bar %d) over %d values" % (loss, C, worst_dev, worst_np, RHO_ULP, probe.size))


def test_non_finite_residuals_give_a_nan_cost(long_vectors, cuda):
    """A NaN, a +inf, a -inf, one at a time, in the first element, the last, and in the grid-stride loop's second lap (index 65 536 of a
    65 537-vector -- its only element there -- and index 65 536 + 7 of a 65 600-vector): the cost is NaN for all five losses (arctan
    alone would turn an infinite residual into a finite cost).  NaN arithmetic, no fault."""
    from deepfly3d_amd import _native

    dv = long_vectors.dv
    rng = np.random.default_rng(12)
    for n, where in ((LAP + 1, (0, LAP)), (LAP + 64, (0, LAP + 7, LAP + 63))):
        base = _up(2.0 * rng.normal(size=n), cuda)
        for code in range(len(bro.LOSSES)):
            assert math.isfinite(dv.robust_cost(base, code, 2.0))
        for i in where:
            assert i < n
            for bad in (float("nan"), float("inf"), float("-inf")):
                v = base.clone()
                v[i] = bad
                for code, loss in enumerate(_native.BA_LOSSES):
                    assert math.isnan(dv.robust_cost(v, code, 2.0)), (loss, n, i, bad)


def test_a_nan_detection_stays_in_its_rows(dials, cuda):
    """One observation of the two-block dial problem gets a NaN detection: its two rows' f (unscaled and scaled) are NaN, and every
    other row's outputs are bit-equal to the run without it."""
    from deepfly3d_amd import _native

    C = dials.C
    d = dials.problems[-1]
    p, nobs = d.p, d.prob.nobs
    for obs in (3, 256):                                     # one in either block
        pt, cam = obs // 2, obs % 2
        px = p["px"].copy()
        px[cam, 0, pt, :] = np.nan
        prob, dv = _device_problem(px, p["intr"], cuda)
        assert prob.nobs == nobs                             # (NaN != 0: the observation is still in the table)
        bad = types.SimpleNamespace(p=p, prob=prob, dv=dv, x=d.x)
        rows = np.zeros(2 * nobs, bool)
        rows[2 * obs : 2 * obs + 2] = True
        for loss in bro.LOSSES:
            code = _native.BA_LOSSES.index(loss)
            clean, got = _run(d, code, C, cuda), _run(bad, code, C, cuda)
            _assert_the_dial_is_right(clean, p)
            assert np.isnan(got.f_true[rows]).all() and np.isnan(got.f[rows]).all()
            for name in ("f_true", "f", "w", "s", "s_c"):
                a, b = getattr(clean, name), getattr(got, name)
                assert np.array_equal(a[~rows].view(np.int64), b[~rows].view(np.int64)), (loss, obs, name)
            others = np.arange(nobs) != obs
            assert np.array_equal(clean.jc[:, :, others].view(np.int64), got.jc[:, :, others].view(np.int64))
            assert np.array_equal(clean.jp[:, :, others].view(np.int64), got.jp[:, :, others].view(np.int64))
