"""CPU checks of the residual dial (tests/ba_robust_dial.py; DESIGN.md section 26, "Sweep"): with the float64 oracle and 50-digit mpmath
alone, every condition tests/test_gpu_ba_robust_sweep.py relies on -- the dial reaches both sides of the clamp of cauchy and arctan,
adjacent numbers straddle it, huber's branch point is hit exactly, the oracle is finite on every row and agrees with exact arithmetic
wherever a rounding does not decide.  Nothing here needs a device."""
import numpy as np
import pytest

import ba_robust_dial as dial
import ba_robust_oracle as bro
from oracle import geometry as og
from oracle.trf_lsmr import eval_blocks

EPS = np.finfo(np.float64).eps


def _rows(loss, C):
    v = dial.values(C)
    return (v,) + dial.oracle_rows(loss, v["f"], C)


@pytest.mark.parametrize("C", dial.F_SCALES)
def test_the_dial_problems_plant_what_they_say(C):
    """The sizes, both signs, the zero point, and -- through the oracle's own evaluation of the problem -- residuals equal to the planted
    values bit for bit and the Jacobian planes that read s out equal to 1."""
    v = dial.values(C)
    n = v["f"].size // 2
    assert np.array_equal(v["f"][:n], -v["f"][n:]) and (v["f"][:n] > 0).all()
    one = v["f"][:n][v["group"][:n] == "one"]
    assert one.size == 65 and one[32] == C and (np.diff(one) > 0).all() and one[33] == np.nextafter(C, np.inf) and one[31] == np.nextafter(C, 0.0)
    probs = dial.problems(C)
    assert tuple(p["nobs"] for p in probs) == dial.NOBS == (2, 254, 256, 258)
    seen = np.concatenate([p["planted"][p["dial"]] for p in probs])
    assert np.isin(v["f"], seen).all()                                # every dial value is in some problem
    for p in probs:
        px, nobs = p["px"], p["nobs"]
        cam_idx, pt_idx, obs_xy, slot = og.build_observations(px)
        assert cam_idx.size == nobs and np.array_equal(cam_idx, np.tile([0, 1], nobs // 2)) and np.array_equal(pt_idx, np.repeat(np.arange(nobs // 2), 2))
        r, Jc, Jp = eval_blocks(p["x"], 2, p["intr"], cam_idx, pt_idx, obs_xy)
        assert np.array_equal(r, p["planted"]), "the dial is wrong"
        assert np.array_equal(np.signbit(r), np.signbit(p["planted"]))
        assert (Jp[:, 0, 0] == 1).all() and (Jp[:, 1, 1] == 1).all() and (Jp[:, 0, 1] == 0).all() and (Jp[:, 1, 0] == 0).all()
        assert (Jc[:, 0, 3] == 1).all() and (Jc[:, 1, 4] == 1).all()
        assert int(p["zero"].sum()) == (4 if nobs > 2 else 0) and (p["planted"][p["zero"]] == 0).all()
        assert not (p["dial"] & p["zero"]).any()
        assert (~p["dial"] & ~p["zero"]).sum() == (0 if nobs == 2 else 2 * nobs - 4 - int(p["dial"].sum())) and (nobs == 2 or (~p["dial"] & ~p["zero"]).any())


@pytest.mark.parametrize("C", dial.F_SCALES)
@pytest.mark.parametrize("loss", ("cauchy", "arctan"))
def test_the_dial_reaches_both_sides_of_the_clamp(loss, C):
    v, z, w, s, fs, clamped = _rows(loss, C)
    with np.errstate(over="ignore", invalid="ignore"):
        s2 = bro.s2_closed(loss, z)
    inside = ~clamped & (s2 > 0) & (s2 < 1e-6)
    print("%s C=%g: %d of %d dial rows clamped, %d unclamped with 0 < s^2 < 1e-6" % (loss, C, int(clamped.sum()), clamped.size, int(inside.sum())))
    assert clamped.any() and inside.sum() >= 20
    # the ladder does what it is for: its unclamped side has s^2 through every decade of (EPS, 1e-6)
    lad = (v["group"] == ("lad_c" if loss == "cauchy" else "lad_a")) & (v["k"] > 0) & (v["f"] > 0)
    decades = np.unique(np.floor(np.log10(s2[lad & inside])))
    assert set(decades) >= set(range(-15, -6)), decades
    assert clamped[(v["group"] == ("lad_c" if loss == "cauchy" else "lad_a")) & (v["k"] < 0)].all()
    # a pair of ADJACENT float64 residuals on opposite sides of the clamp, for either sign
    grp = "one" if loss == "cauchy" else "arctan"
    for sign in (1, -1):
        sel = (v["group"] == grp) & (np.sign(v["f"]) == sign)
        f, c = v["f"][sel], clamped[sel]
        assert (np.diff(v["k"][sel]) == 1).all() and np.array_equal(np.abs(f[1:]), np.nextafter(np.abs(f[:-1]), np.inf))
        assert (c[1:] != c[:-1]).any(), (loss, C, sign)


@pytest.mark.parametrize("C", dial.F_SCALES)
def test_the_dial_hits_hubers_branch_point(C):
    """Some row has z == 1.0 exactly, and the rows next to it take the numbers next to 1 that z can take.  z == nextafter(1, 2) = 1 + EPS,
    which one would ask for first, is not among them, for any f and C: z is the rounded square of a float64 q, q <= 1 gives z <= 1, and
    the smallest q above 1 is 1 + EPS, whose square 1 + 2 EPS + EPS^2 rounds to 1 + 2 EPS.  So the nearest z above 1 is 1 + 2 EPS, and
    that one is required here; asserted below on every dial row rather than taken on trust."""
    v, z, w, s, fs, clamped = _rows("huber", C)
    assert (z == 1.0).any()
    assert not (z == np.nextafter(1.0, 2.0)).any()
    assert (z == 1.0 + 2 * EPS).any() and (z[z > 1].min() == 1.0 + 2 * EPS)
    assert ((z < 1) & (z >= 1 - 4 * EPS)).any()
    assert not clamped[z <= 1].any() and clamped[z > 1].all()
    assert (w[z <= 1] == 1).all() and (w[z > 1] < 1).all()


@pytest.mark.parametrize("C", dial.F_SCALES)
@pytest.mark.parametrize("loss", bro.LOSSES)
def test_the_oracle_is_finite_and_exact_arithmetics_where_no_rounding_decides(loss, C):
    """w, s and f w / s of the oracle are finite on every dial row (fill and zeros too).  Against 50-digit arithmetic at the exact
    (f / C)^2: w within 8 EPS -- arctan's chain is the longest: q, z, z^2, 1 + z^2 and the quotient, half an ulp each, the error of q
    counted four times and that of z twice, nine half-ulps = 4.5 EPS -- on every row, and the clamp's decision on every row whose exact
    s^2 is further than 1e-9 from EPS.  The rows nearer than that are the ones a rounding can decide: there the float64 oracle IS the
    specification (scipy is float64 too)."""
    import mpmath as mp

    z, w, s, fs, clamped = dial.oracle_rows(loss, dial.all_planted(C), C)
    assert np.isfinite(w).all() and np.isfinite(s).all() and np.isfinite(fs).all() and (s >= 2.0**-26).all()
    v, z, w, s, fs, clamped = _rows(loss, C)
    assert np.isfinite(w).all() and np.isfinite(s).all() and np.isfinite(fs).all()
    near = decided = 0
    worst = 0.0
    for i, f in enumerate(v["f"]):
        w_mp, s2_mp = dial.mp_row(loss, f, C)
        worst = max(worst, float(abs(mp.mpf(float(w[i])) - w_mp) / w_mp))
        d = abs(s2_mp - mp.mpf(EPS))
        if d > 1e-9:
            assert bool(clamped[i]) == bool(s2_mp <= EPS), (loss, C, f)
        else:
            near += 1
            # (the error of the computed s^2 next to its zero: z carries 1.5 EPS, arctan's 3 z^2 ~ 1 then 3.5 EPS, times 9 / 16: 2 EPS;
            # a row of the 'special' group is near EPS only because its s^2 is all but 0)
            decided += abs(dial.mp_z(f, C) - 1) <= 4 * EPS if loss == "huber" else d <= 2 * EPS and v["group"][i] != "special"
    print("%s C=%g: w against 50 digits: %.2f EPS at worst (bar 8); %d of %d dial rows have the exact s^2 within 1e-9 of EPS, %d of them within 2 EPS (huber: z within 4 EPS of 1)"
          % (loss, C, worst / EPS, near, v["f"].size, decided))
    assert worst <= 8 * EPS
    if loss != "linear":
        assert near >= 1
    if loss in ("huber", "cauchy", "arctan"):      # (soft_l1's s^2 reaches EPS at z = 2.7e10 only; none of its rows hangs on a rounding)
        assert decided >= 1


def test_the_rho_probe_covers_what_it_is_for():
    for C in dial.F_SCALES:
        f = dial.rho_probe(C)
        z = (f / C) ** 2
        assert 30 <= f.size <= 80
        assert (z == 1).any() and (z == 1 + 2 * EPS).any() and (z == 0).any() and (z > 1e100).any() and (f < 0).any()
        assert np.signbit(f[-1]) and f[-1] == 0 and not np.signbit(f[-2])
