"""GPU sweep of the constant-length leg fit's damped branch (csrc/leg_fit.hip, DESIGN.md section 15, "swept"): ops.fit_legs and
df3d_leg_fit on the families of tests/leg_fit_cases.py, whose trials are rejected at a pivot and on cost, whose lambda climbs and
comes back, whose legs run out of iterations, stall, tie and sit on thresholds, against the float64 oracle tests/leg_fit_oracle.py;
over the sizes at which the launch geometry changes; and bit for bit against itself: a lane's arithmetic is its own, wherever it sits
in a wave and whenever its neighbours leave the loop.

Bars: leg_fit_cases.bars(), ten times the oracle's own path-to-path difference and never below the existing bars times the coordinate
scale; tests/test_leg_fit_cases_host.py certifies the families and pins those differences.  (status, iters) may differ from the oracle on
at most FLIP_CAP of a family's fitted legs, never on a leg that is not fitted or whose lengths overflow; the legs that differ are printed.
Every comparison prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import leg_fit_cases as lc
import leg_fit_oracle as lo

pytestmark = pytest.mark.gpu

NAMES = list(lc.families())
SIZES = (1, 10, 11, 24, 64, 65, 75)   # lane 64 is frame 10's leg 4; frame 64 opens a second block; T = 65 leaves a wave of 6 lanes
SWEPT = ("noisy", "long_offset", "short_free", "compressed", "compressed_free", "stalled", "edges", "shifted", "mixed", "mixed_free")
OTHERS = [j for j in range(38) if j not in lc.LEG_JOINTS]


def _dev(cuda, a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(cuda)   # a copy: the families are read-only


def _fit(cuda, fam):
    from deepfly3d_amd import ops

    r = ops.fit_legs(_dev(cuda, fam.X), fam.L, "per_frame" if fam.A is None else fam.A, max_iter=fam.max_iter)
    return tuple(a.cpu().numpy() for a in (r.status, r.iters, r.points, r.cost))


def _against_oracle(cuda, name, fam):
    """The kernel on `fam`, the family `name` itself or its frames repeated to another size.  The cap on differing legs is the family's:
    FLIP_CAP of its fitted legs, counted in distinct legs of the family however often the size repeats them."""
    base = lc.families()[name]
    got = _fit(cuda, fam)
    want = lc.fit_family(fam)
    status, iters, pts, cost = got
    assert status.dtype == np.int32 and iters.dtype == np.int32 and pts.shape == fam.X.shape and cost.shape == (len(fam.X), 6)
    fitted = want.status != lo.NOT_FITTED
    firm = ~fitted | lc.overflow_legs(fam)[None, :]                 # no flip allowed here
    differ, dp, dc = lc.compare_fits(fam, got, (want.status, want.iters, want.points, want.cost))
    point_bar, cost_bar = lc.bars(name)
    cap = int(lc.FLIP_CAP * (lc.fit(name).status != lo.NOT_FITTED).sum())
    flipped = {(int(t) % len(base.X), int(leg)) for t, leg in np.argwhere(differ)}
    print(f"{name}, T = {len(fam.X)}: points off by {dp:.3e} mm per unit of scale (bar {point_bar:.3e}), cost by {dc:.3e} relative (bar {cost_bar:.3e}); "
          f"{len(flipped)} of the family's legs differ in (status, iters) (cap {cap}), at {int(differ.sum())} of {int(fitted.sum())} fitted lanes")
    for t, leg in np.argwhere(differ):
        print(f"    frame {t} leg {leg}: kernel ({status[t, leg]}, {iters[t, leg]}), oracle ({want.status[t, leg]}, {want.iters[t, leg]}), "
              f"{len(want.traces[t][leg])} passes")
    assert np.array_equal(status[firm], want.status[firm]) and np.array_equal(iters[firm], want.iters[firm])
    for t, leg in np.argwhere(~fitted):                               # the input's bits, NaN cost, (-1, -1)
        j = lo.leg_joints(leg)
        assert pts[t, j].tobytes() == fam.X[t, j].tobytes() and np.isnan(cost[t, leg]) and iters[t, leg] == -1
    assert pts[:, OTHERS].tobytes() == fam.X[:, OTHERS].tobytes()
    assert len(flipped) <= cap and dp <= point_bar and dc <= cost_bar


# ------------------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", NAMES)
def test_family_against_the_oracle(native_lib, cuda, name):
    _against_oracle(cuda, name, lc.families()[name])


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("name", SWEPT)
def test_sizes(native_lib, cuda, name, T):
    _against_oracle(cuda, name, lc.tiled(lc.families()[name], T))


def test_named_legs_end_as_the_model_says(native_lib, cuda):
    """The legs whose decision has a wide margin, (status, iters) exactly: the tie at a step of 0.85 TOL (a basis from the highest
    tied index gives (0, 2)), LAMBDA_MAX itself tried (lam >= LAMBDA_MAX as the stall test gives (2, 0)), the finite stall, the
    thresholds either side of TINY, the overflow leg."""
    status, iters, _, cost = _fit(cuda, lc.families()["tie_step"])
    assert (status[lc.TIE_SENSITIVE], iters[lc.TIE_SENSITIVE]) == (lo.CONVERGED, 1)
    status, iters, _, cost = _fit(cuda, lc.families()["edges"])
    want = {"lambda_max_tried": (lo.CONVERGED, 1), "finite_stall": (lo.STALLED, 0), "below_tiny": (lo.NOT_FITTED, -1), "straight": (lo.CONVERGED, 1),
            "too_long": (lo.CONVERGED, 1), "antiparallel": (lo.CONVERGED, 1)}
    got = {k: (int(status[lc.EDGE_LEGS[k]]), int(iters[lc.EDGE_LEGS[k]])) for k in lc.EDGE_LEGS}
    print(got)
    assert all(got[k] == v for k, v in want.items()) and got["above_tiny"][0] == lo.CONVERGED and got["tip_on_anchor"][0] == lo.CONVERGED
    assert np.isfinite(cost[lc.EDGE_LEGS["finite_stall"]])
    status, iters, _, cost = _fit(cuda, lc.families()["stalled"])
    assert (status[:, lc.STALLED_LEG] == lo.STALLED).all() and (iters[:, lc.STALLED_LEG] == 0).all() and (cost[:, lc.STALLED_LEG] == np.inf).all()


# ------------------------------------------------------------------------------------------------------------------ bit for bit
def _raw(lib, cuda, X, L, A, max_iter=lo.MAX_ITER, in_place=False, guard=0):
    """df3d_leg_fit itself on sentinel-filled buffers: (out [T, 38, 3], cost [T, 6], info [T, 6, 2]) as numpy, with `guard` words either
    side of each checked to be untouched."""
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    T, sentinel = len(X), -12345.678
    L = np.ascontiguousarray(L, dtype=np.float64)
    A = None if A is None else np.ascontiguousarray(A, dtype=np.float64)
    Xd = _dev(cuda, X)
    n = T * 114
    out = torch.full((guard + n + guard,), sentinel, dtype=torch.float64, device=cuda)
    cost = torch.full((guard + T * 6 + guard,), sentinel, dtype=torch.float64, device=cuda)
    info = torch.full((guard + T * 12 + guard,), -77, dtype=torch.int32, device=cuda)
    o = Xd if in_place else out[guard:guard + n]
    rc = lib.df3d_leg_fit(Xd.data_ptr(), T, ptr(L), None if A is None else ptr(A), max_iter, o.data_ptr(), cost[guard:guard + T * 6].data_ptr(),
                          info[guard:guard + T * 12].data_ptr(), None)
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()
    if guard:
        for buf, m, s in ((out, n, sentinel), (cost, T * 6, sentinel), (info, T * 12, -77)):
            assert (buf[:guard] == s).all() and (buf[guard + m:] == s).all()
    return (o.view(T, 38, 3).cpu().numpy(), cost[guard:guard + T * 6].view(T, 6).cpu().numpy(), info[guard:guard + T * 12].view(T, 6, 2).cpu().numpy())


def _same_legs(a, b, frames_a, frames_b):
    for x, y in zip(a, b):
        x, y = x[frames_a], y[frames_b]
        if x.ndim == 3 and x.shape[1] == 38:
            x, y = x[:, lc.LEG_JOINTS], y[:, lc.LEG_JOINTS]
        if x.tobytes() != y.tobytes():
            return False
    return True


@pytest.mark.parametrize("name", ["mixed", "mixed_free"])
def test_a_leg_is_the_same_bits_wherever_it_sits(native_lib, cuda, name):
    """Alone in a T = 1 call, or at frame 0, 10, 63, 64, T - 1 of the mixed batch whose waves hold lanes that leave at pass 0, ~5, 17
    and beyond 20; out of place or in place."""
    fam = lc.tiled(lc.families()[name], 75)
    batch = _raw(native_lib, cuda, fam.X, fam.L, fam.A)
    in_place = _raw(native_lib, cuda, fam.X, fam.L, fam.A, in_place=True)
    assert _same_legs(batch, in_place, slice(None), slice(None))
    assert in_place[0][:, OTHERS].tobytes() == fam.X[:, OTHERS].tobytes()
    info = batch[2]
    assert {int(s) for s in np.unique(info[..., 0])} >= {lo.NOT_FITTED, lo.CONVERGED, lo.STALLED}
    for t in (0, 10, 63, 64, 74):
        for place in (False, True):
            alone = _raw(native_lib, cuda, fam.X[t:t + 1], fam.L, fam.A, in_place=place)
            assert _same_legs(alone, batch, slice(None), slice(t, t + 1)), (t, place)
    # a shorter batch: the same frames in other waves' company
    for T in (11, 65):
        part = _raw(native_lib, cuda, fam.X[75 - T:], fam.L, fam.A)   # frame t of the part is frame 75 - T + t of the batch: other lanes
        assert _same_legs(part, batch, slice(None), slice(75 - T, 75)), T


def test_an_anchor_table_of_the_frames_own_joints_changes_no_bit(native_lib, cuda):
    fam = lc.families()["mixed_free"]
    for t in (0, 1, 3, 6):
        X = fam.X[t:t + 1]
        own = np.ascontiguousarray(X[0, lo.COXAE])
        assert np.isfinite(own).all()
        free, anchored = _raw(native_lib, cuda, X, fam.L, None), _raw(native_lib, cuda, X, fam.L, own)
        assert _same_legs(free, anchored, slice(None), slice(None)), t


def test_two_runs_give_the_same_bits_also_on_a_side_stream(native_lib, cuda):
    from deepfly3d_amd import ops

    fam = lc.tiled(lc.families()["mixed"], 75)
    Xd = _dev(cuda, fam.X)

    def run():
        r = ops.fit_legs(Xd, fam.L, fam.A)
        torch.cuda.synchronize()
        return r.points.cpu().numpy().tobytes(), r.cost.cpu().numpy().tobytes(), r.status.cpu().numpy().tobytes(), r.iters.cpu().numpy().tobytes()

    first = run()
    assert run() == first
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        assert run() == first
    raw = _raw(native_lib, cuda, fam.X, fam.L, fam.A)
    assert raw[0][:, lc.LEG_JOINTS].tobytes() == np.frombuffer(first[0]).reshape(75, 38, 3)[:, lc.LEG_JOINTS].tobytes() and raw[1].tobytes() == first[1]


def test_guard_words_and_the_other_joints_at_65_frames(native_lib, cuda):
    for name in ("mixed", "mixed_free"):
        fam = lc.tiled(lc.families()[name], 65)
        out, cost, info = _raw(native_lib, cuda, fam.X, fam.L, fam.A, guard=16)   # checks the guard words
        assert (out[:, OTHERS] == -12345.678).all()                               # the eight other joints are never written
        assert not (out[:, lc.LEG_JOINTS] == -12345.678).any() and not (info == -77).any()
        want = lc.fit_family(fam)
        assert np.array_equal(info[..., 0] == lo.NOT_FITTED, want.status == lo.NOT_FITTED)
