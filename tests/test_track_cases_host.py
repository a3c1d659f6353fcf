"""CPU certificate of the families tests/test_gpu_track_sweep.py runs on the device (tests/track_cases.py, DESIGN.md section 22, "swept"):
every condition the device tests rely on is asserted here on the oracle alone, with the measured value printed, and each mutant of the
model -- a rule changed in this file's own copy of the oracle -- changes the result on the family that is meant to see it."""
import time

import numpy as np
import pytest

import track_cases as tc
import track_oracle as to

DEFAULTS = (to.TAU, to.W_MOTION, to.W_VALUE)


# ------------------------------------------------------------------------------------------------------------------ a copy that can be wrong
def model(count, pts, val, image_hw, tau=to.TAU, w_motion=to.W_MOTION, w_value=to.W_VALUE, clamp=True, rounding=np.rint, swap_hw=False,
          placeholder_pair=None, count_le=False, last_highest=False, back_highest=False):
    """track_oracle.solve restated frame by frame; with the defaults it is the oracle (asserted wherever a mutant is used), and every
    keyword changes one rule."""
    def q(x):
        return rounding(np.asarray(x, np.float64) * to.SCALE).astype(np.int64)

    C, T, J = np.asarray(count).shape
    count, pts, val = to._chains(count), to._chains(pts), to._chains(val)
    N, K = C * J, val.shape[-1]
    k_of = np.arange(K)
    real = ((k_of <= count[..., None]) if count_le else (k_of < count[..., None])) & np.isfinite(val) & np.isfinite(pts).all(axis=-1)
    placeholder = ~real.any(axis=-1)
    v = np.where(real, val, 0.0).astype(np.float64)
    best = np.where(real, v, -np.inf).max(axis=-1, initial=-np.inf)
    gap = np.where(real, np.where(placeholder, 0.0, best)[..., None] - v, 0.0)
    qu = np.where(real, q(w_value * (np.minimum(gap, 1.0) if clamp else gap)), to.INF)
    valid = real.copy()
    valid[..., 0] |= placeholder
    qu[..., 0] = np.where(placeholder, 0, qu[..., 0])
    H, W = (image_hw[1], image_hw[0]) if swap_hw else image_hw
    rows = np.where(real, pts[..., 0], 0.0).astype(np.float64) * float(H)
    cols = np.where(real, pts[..., 1], 0.0).astype(np.float64) * float(W)
    tt = float(tau) * float(tau)
    q_hold = q(w_motion) if placeholder_pair is None else np.int64(placeholder_pair)
    back = np.zeros((T, N, K), np.int64)
    a = qu[0].copy()
    lanes = np.arange(N)[:, None]
    for t in range(1, T):
        dr = rows[t, :, None, :] - rows[t - 1, :, :, None]
        dc = cols[t, :, None, :] - cols[t - 1, :, :, None]
        qd = q(w_motion * np.minimum(dr * dr + dc * dc, tt) / tt)
        qd = np.where((placeholder[t] | placeholder[t - 1])[:, None, None], q_hold, qd)
        qd = np.where(valid[t, :, None, :] & valid[t - 1, :, :, None], qd, 0)
        cand = np.minimum(a[:, :, None] + qd, to.INF)
        arg = K - 1 - cand[:, ::-1].argmin(axis=1) if back_highest else cand.argmin(axis=1)
        back[t] = arg
        a = np.minimum(qu[t] + cand[lanes, arg, k_of], to.INF)
    k = K - 1 - a[:, ::-1].argmin(axis=-1) if last_highest else a.argmin(axis=-1)
    cost = a.min(axis=-1)
    choice = np.zeros((T, N), np.int32)
    for t in range(T - 1, -1, -1):
        choice[t] = k
        k = back[t, np.arange(N), k]
    return np.ascontiguousarray(np.moveaxis(choice.reshape(T, C, J), 0, 1)), cost.reshape(C, J)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def sees(peaks, image_hw, params, **mutation):
    """The unmutated copy is the oracle on this input, and the mutant is not."""
    want = to.solve(*peaks, image_hw, *params)
    assert same(model(*peaks, image_hw, *params), want)
    return not same(model(*peaks, image_hw, *params, **mutation), want)


# ------------------------------------------------------------------------------------------------------------------ scattered
def scattered_figures(peaks, image_hw=tc.IMAGE_HW):
    """The six figures of a `scattered` input under the default parameters, as fractions (None where there is nothing to count)."""
    T = peaks[0].shape[1]
    valid, placeholder, rows, cols, qu = to.slots(*peaks, image_hw)
    real = valid & ~placeholder[..., None]
    v = np.where(real, to._chains(peaks[2]), -np.inf).astype(np.float64)
    gap = (v.max(axis=-1, keepdims=True) - v)[real]
    choice, cost = to.solve(*peaks, image_hw)
    flat = to._chains(choice)                                            # [T, N]
    off_best = np.take_along_axis(qu, flat[..., None].astype(np.int64), axis=-1)[..., 0][~placeholder] > 0
    out = dict(real=int(real.sum()), above=float((gap > 1.0).mean()), inside=float(((gap > 0.0) & (gap < 1.0)).mean()),
               off_best=float(off_best.mean()), between=None, at_limit=None,
               motion_matters=not same((choice, cost), to.solve(*peaks, image_hw, w_motion=0.0)))
    if T > 1:
        qd = to.pair_costs(valid, placeholder, rows, cols, 1, T)
        pairs = qd[real[1:, :, None, :] & real[:-1, :, :, None]]
        qm = int(to.quantise(to.W_MOTION))
        out.update(pairs=int(pairs.size), between=float(((pairs > 0) & (pairs < qm)).mean()), at_limit=float((pairs == qm).mean()))
    return out


@pytest.fixture(scope="module")
def instances():
    return tc.scattered_instances()


def test_every_scattered_instance_is_in_general_position(instances):
    """Per instance the device runs, under the default parameters: a fifth of the pair costs between real slots strictly inside (0, q(w_m)),
    a fifth at q(w_m); a tenth of the valid slots with v_best - v > 1, three tenths strictly inside (0, 1); the solution off the frame's
    best value in a tenth of the non-placeholder frames and not the solution without a motion term.  One frame has no pair cost and its
    solution IS the best value: there only the two value conditions can hold, and they are asserted.  The weights family runs these inputs
    under other parameters; what it needs of them is certified in test_weights_at_their_ends."""
    assert len(instances) == 2 * len(tc.MANY_CHAINS) + len(tc.WEIGHTS_T) + 2 * 28 + 1
    lowest = {}
    for name, peaks in instances.items():
        f = scattered_figures(peaks)
        print(name, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in f.items()})
        assert f["above"] >= 0.10 and f["inside"] >= 0.30, name
        if peaks[0].shape[1] > 1:
            assert f["between"] >= 0.20 and f["at_limit"] >= 0.20 and f["off_best"] >= 0.10 and f["motion_matters"], name
        else:
            assert f["between"] is None and f["off_best"] == 0.0 and not f["motion_matters"]
        for k in ("above", "inside", "between", "at_limit", "off_best"):
            if f[k] is not None and peaks[0].shape[1] > 1:
                lowest[k] = min(lowest.get(k, 1.0), f[k])
    print("the lowest of each figure over the instances of more than one frame:", {k: round(v, 3) for k, v in lowest.items()})


def test_scattered_holds_what_its_docstring_says():
    count, pts, val = tc.wide_grid()
    assert count.dtype == np.int32 and pts.dtype == np.float32 and val.dtype == np.float32
    assert count.min() == tc.INT_MIN and count.max() == tc.INT_MAX
    inner = count[(count != tc.INT_MIN) & (count != tc.INT_MAX)]
    assert inner.min() == -3 and inner.max() == tc.WIDE_GRID["K"] + 3
    finite = pts[np.isfinite(pts)]
    assert (finite < 0.0).any() and (finite > 1.0).any() and np.abs(finite).max() >= 1e30
    assert (val == tc.SUBNORMAL).any() and 0.0 < float(tc.SUBNORMAL) < np.finfo(np.float32).tiny and np.isneginf(val).any()
    assert np.isnan(val).any() and np.isposinf(val).any() and np.isnan(pts[..., 0]).any() and np.isneginf(pts[..., 1]).any()
    ok = val[np.isfinite(val)]
    assert -1.5 < ok.min() < -0.5 and 2.4 < ok.max() <= 2.5
    again = tc.wide_grid()
    assert all(a.tobytes() == b.tobytes() for a, b in zip((count, pts, val), again))
    # the planted values are in every instance that has room for them
    for name, (count, pts, val) in tc.scattered_instances().items():
        assert (count == tc.INT_MIN).any() and (count == tc.INT_MAX).any() and (val == tc.SUBNORMAL).any() and np.isneginf(val).any(), name


def test_coordinates_over_the_whole_image_would_be_useless():
    """What `scattered` is built to avoid: with the slots anywhere in the image nearly every pair cost is w_m."""
    rng = np.random.default_rng(0)
    count = np.full((2, 37, 3), 4, np.int32)
    peaks = (count, rng.random((2, 37, 3, 4, 2), dtype=np.float32), rng.uniform(-0.5, 2.5, (2, 37, 3, 4)).astype(np.float32))
    f = scattered_figures(peaks)
    print(f)
    assert f["at_limit"] > 0.95 and f["between"] < 0.05


# ------------------------------------------------------------------------------------------------------------------ many chains
def test_many_chains_tell_their_chains_apart():
    for C, J in tc.MANY_CHAINS:
        peaks = tc.many_chains(C, J, 37)
        choice, cost = to.solve(*peaks, tc.IMAGE_HW)
        distinct = len(set(cost.ravel().tolist()))
        print(f"{C} x {J}, T = 37: {distinct} distinct costs of {C * J}; the last chain off slot 0 in {int((choice[-1, :, -1] != 0).sum())} frames")
        assert distinct == C * J and choice[-1, :, -1].any()
        one = tc.many_chains(C, J, 1)
        choice, cost = to.solve(*one, tc.IMAGE_HW)
        print(f"{C} x {J}, T = 1: the last chain chooses slot {int(choice[-1, 0, -1])}, {int((choice != 0).sum())} chains off slot 0")
        assert not cost.any() and choice[-1, 0, -1] != 0     # one frame: the best value costs nothing; the choice still tells chains apart
        assert len({c.tobytes() for c in to._chains(peaks[2])[0]}) == C * J
    assert [C * J for C, J in tc.MANY_CHAINS] == [15, 16, 17, 255, 256, 257, 513]
    assert -(-37 // 5) == 8 and 513 * 8 > 256 * 8


# ------------------------------------------------------------------------------------------------------------------ half-way costs
def _halfway_products(K):
    tau, wm, wv = tc.HALFWAY_PARAMS
    peaks = tc.halfway(600 + K, K)
    valid, placeholder, rows, cols, qu = to.slots(*peaks, tc.HALFWAY_HW, wv)
    real = valid & ~placeholder[..., None]
    dr = rows[1:, :, None, :] - rows[:-1, :, :, None]
    dc = cols[1:, :, None, :] - cols[:-1, :, :, None]
    pair = (wm * np.minimum(dr * dr + dc * dc, tau * tau) / (tau * tau) * to.SCALE)[real[1:, :, None, :] & real[:-1, :, :, None]]
    v = np.where(real, to._chains(peaks[2]), -np.inf).astype(np.float64)
    unary = (wv * np.minimum(v.max(axis=-1, keepdims=True) - v, 1.0) * to.SCALE)[real]
    return peaks, pair, unary


@pytest.mark.parametrize("K", tc.HALFWAY_K)
def test_halfway_costs_are_halfway(K):
    peaks, pair, unary = _halfway_products(K)
    assert tc.HALFWAY_PARAMS == (32.0, 2.0 ** -11, 2.0 ** -19) and peaks[0].shape == (2, 70, 3)
    for name, x in (("pair", pair), ("unary", unary)):
        assert np.array_equal(x * 2.0, np.rint(x * 2.0))                  # every product is exact: a whole number of halves
        half = x[x != np.floor(x)]
        share, parts = half.size / x.size, np.floor(half).astype(np.int64) % 2
        print(f"K = {K}, {name}: {x.size} costs, {share:.3f} at x.5, {int((parts == 0).sum())} with an even and {int((parts == 1).sum())} with an odd "
              f"integer part")
        assert share >= 0.25 and (parts == 0).any() and ((parts == 1).any() or name == "pair")
    # an odd sum of two squares is 1 mod 4, so a pair cost at x.5 is (4 m + 1) / 2 = 2 m + 0.5: its integer part is ALWAYS even on whole
    # pixels, rint and truncation agree on it, and floor(x + 0.5) does not.  Odd integer parts, where truncation and rint part, come
    # from the unary costs alone (1.5 -> 2)
    assert not (np.floor(pair[pair != np.floor(pair)]).astype(np.int64) % 2).any() and (unary == 1.5).any() and (unary == 0.5).any()
    assert np.array_equal(pair * 2.0, np.rint(pair * 2.0)) and pair.max() == 512.0
    choice, cost = to.solve(*peaks, tc.HALFWAY_HW, *tc.HALFWAY_PARAMS)
    assert choice.any() and cost.all()


# ------------------------------------------------------------------------------------------------------------------ weights
def test_weights_at_their_ends():
    assert tc.WEIGHTS[0] == (30.0, 1024.0, 1024.0) and tc.WEIGHTS[4] == (30.0, 2.0 ** -21, 2.0 ** -21)
    peaks = tc.weights_case(70)
    choice, cost = to.solve(*peaks, tc.IMAGE_HW, *tc.WEIGHTS[0])
    valid, placeholder, rows, cols, qu = to.slots(*peaks, tc.IMAGE_HW, 1024.0)
    qd = to.pair_costs(valid, placeholder, rows, cols, 1, 70, 30.0, 1024.0)
    print(f"(30, 1024, 1024), T = 70: the costs are {sorted((cost.ravel() / 2.0 ** 31).round(2).tolist())} x 2^31; {int((qd == 2 ** 30).sum())} pair-table "
          f"entries of {qd.size} are 2^30")
    assert (cost > 2 ** 31).all() and (qd == 2 ** 30).any() and qd.max() == 2 ** 30 and qu[valid].max() == 2 ** 30
    for T in tc.WEIGHTS_T:
        peaks = tc.weights_case(T)
        found = {}
        for params in tc.WEIGHTS:
            choice, cost = to.solve(*peaks, tc.IMAGE_HW, *params)
            found[params] = (choice, cost)
            print(f"T = {T}, (tau, w_m, w_v) = {params}: {int((choice != 0).sum())} of {choice.size} choices off slot 0, costs up to {int(cost.max())}")
        assert len({c.tobytes() for c, _ in found.values()}) >= 4              # the ends are different problems
        zero = found[tc.WEIGHTS[4]]
        assert to.quantise(2.0 ** -21) == 0 and not zero[1].any() and zero[0].any()   # every path costs 0: the tie rule alone, and it chooses
        valid = to.slots(*peaks, tc.IMAGE_HW)[0]
        lowest = np.moveaxis(valid.argmax(axis=-1).reshape(T, 2, 3), 0, 1)
        assert np.array_equal(zero[0], lowest)                                   # ... the lowest valid slot of every frame
        assert to.quantise(3 * 2.0 ** -21) == 2
        tiny, huge = found[tc.WEIGHTS[2]], found[tc.WEIGHTS[3]]
        steps = (tiny[1] >> 20) << 20
        assert ((tiny[1] - steps) < 1 << 20).all() and (steps >= (T - 1) << 19).all()   # tau below every jump: most steps cost all of w_m
        assert (huge[1] < T << 20).all() and (huge[1] < tiny[1]).all()                  # tau above every jump inside the image


# ------------------------------------------------------------------------------------------------------------------ placeholders
@pytest.mark.parametrize("B", tc.SWEEP_BLOCKS)
def test_placeholders_by_design(B):
    frames = tc.placeholder_frames(B)
    T = tc.T_DESIGNED
    assert frames.shape == (len(tc.PLACEHOLDER_PATTERNS), T) == (8, 70)
    assert frames[0].all() and frames[1].tolist() == [True] + [False] * 69 and frames[2].tolist() == [False] * 69 + [True]
    assert np.nonzero(frames[4])[0].tolist() == list(range(16, 32)) and np.nonzero(frames[5])[0].tolist() == list(range(16, 48))
    assert frames[6].sum() == 35 and not frames[7][30] and frames[7][29] and frames[7][31]
    edges = sorted({t for b in range(1, -(-T // B)) for t in (b * B - 1, b * B)})
    assert np.nonzero(frames[3])[0].tolist() == edges and (len(edges) >= 2 or B == 70)
    peaks = tc.placeholders(50 + B, B)
    placeholder = to.slots(*peaks, tc.IMAGE_HW)[1]
    assert np.array_equal(placeholder.T, frames)                               # the patterns, and no placeholder besides them
    choice, cost = to.solve(*peaks, tc.IMAGE_HW)
    qm = int(to.quantise(to.W_MOTION))
    print(f"B = {B}: costs {cost[0].tolist()}, choices off slot 0 per pattern {(choice[0] != 0).sum(axis=0).tolist()}")
    assert cost[0, 0] == (T - 1) * qm and not choice[0, :, 0].any()
    assert not choice[0][frames.T].any()
    assert all(choice[0, :, j].any() for j in range(1, 8) if (~frames[j]).sum() >= 30)   # the other frames do choose
    for made in (peaks[0] == 0, peaks[0] == tc.INT_MIN, np.isnan(peaks[2]).all(axis=-1) & (peaks[0] == 4)):
        assert made.any() and placeholder.T[made[0].T].all()                     # the three ways to make one


# ------------------------------------------------------------------------------------------------------------------ designed ties
@pytest.mark.parametrize("B", tc.SWEEP_BLOCKS)
def test_designed_ties(B):
    count, pts, val, wanted = tc.designed_ties(B)
    T = tc.T_DESIGNED
    frames = tc.tie_frames(B)
    nb = -(-T // B)
    assert T - 1 in frames and B - 1 in frames and (B in frames or B >= T) and 3 in frames      # a block's last frame and a block's first
    assert any(t % B == 0 for t in frames) and any(t % B == B - 1 or t == T - 1 for t in frames) and nb >= 2
    choice, cost = to.solve(count, pts, val, tc.IMAGE_HW)
    assert not cost.any() and np.array_equal(choice, wanted) and wanted.sum() == 2 * len(frames)
    valid, placeholder, _, _, qu = to.slots(count, pts, val, tc.IMAGE_HW)
    assert not qu[valid].any() and not placeholder.any()                          # every valid slot is free: all paths over them cost 0


# ------------------------------------------------------------------------------------------------------------------ brute force
def test_small_instances_against_brute_force():
    cases = {"scattered": (tc.scattered(11, 1, 7, 2, 4), tc.IMAGE_HW, DEFAULTS),
             "many chains": (tc.many_chains(15, 1, 1), tc.IMAGE_HW, DEFAULTS),
             "half-way": (tc.halfway(603, 3, C=1, T=8, J=2), tc.HALFWAY_HW, tc.HALFWAY_PARAMS),
             "placeholders": (tc.placeholders(12, 3, K=3, T=9), tc.IMAGE_HW, DEFAULTS),
             "designed ties": (tc.designed_ties(3, T=8)[:3], tc.IMAGE_HW, DEFAULTS),
             "odd blocks": (tc.scattered(13, 2, 9, 3, 3), tc.IMAGE_HW, DEFAULTS)}
    for n, params in enumerate(tc.WEIGHTS):
        cases[f"weights {params}"] = (tc.scattered(14 + n, 1, 5, 2, tc.WEIGHTS_K), tc.IMAGE_HW, params)
    t0 = time.perf_counter()
    for name, (peaks, hw, params) in cases.items():
        K, T = peaks[2].shape[-1], peaks[0].shape[1]
        assert K ** T <= 10 ** 6, name
        assert same(to.solve(*peaks, hw, *params), to.brute_force(*peaks, hw, *params)), name
    print(f"{len(cases)} cases against every path: {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_the_families_see_the_mutants_they_are_meant_for():
    scattered = tc.odd_blocks_case(3, 67), tc.IMAGE_HW, DEFAULTS
    halfway = [(tc.halfway(600 + K, K), tc.HALFWAY_HW, tc.HALFWAY_PARAMS) for K in tc.HALFWAY_K]
    ties = [(tc.designed_ties(B)[:3], tc.IMAGE_HW, DEFAULTS) for B in tc.SWEEP_BLOCKS]
    zero_weights = [(tc.weights_case(T), tc.IMAGE_HW, tc.WEIGHTS[4]) for T in tc.WEIGHTS_T]
    holders = [(tc.placeholders(50 + B, B), tc.IMAGE_HW, DEFAULTS) for B in tc.SWEEP_BLOCKS]
    assert sees(*scattered, clamp=False)
    assert sees(*scattered, swap_hw=True)
    assert sees(*scattered, count_le=True)
    for case in halfway:
        assert sees(*case, rounding=lambda x: np.floor(x + 0.5))
        assert sees(*case, rounding=np.trunc)
    for case in holders:
        assert sees(*case, placeholder_pair=0)
    for case in ties + zero_weights:
        assert sees(*case, last_highest=True)
        assert sees(*case, back_highest=True)
    # and every scattered instance of more than one frame sees the three that are its own
    for name, peaks in tc.scattered_instances().items():
        if peaks[0].shape[1] >= 14:
            seen = [sees(peaks, tc.IMAGE_HW, DEFAULTS, **m) for m in (dict(clamp=False), dict(swap_hw=True), dict(count_le=True))]
            assert all(seen), (name, seen)


def test_the_references_are_quick():
    t0 = time.perf_counter()
    to.solve(*tc.wide_grid(), tc.IMAGE_HW)
    wide = time.perf_counter() - t0
    t0 = time.perf_counter()
    to.solve(*tc.odd_blocks_case(16, 1027), tc.IMAGE_HW)
    long = time.perf_counter() - t0
    print(f"the oracle: {wide:.2f} s on the wide grid, {long:.2f} s on 1 027 frames of K = 16")
    assert wide < 1.0 and long < 1.0
