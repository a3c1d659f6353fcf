"""GPU tests of the behaviour map's large-N routes ("tested sizes"): the later trips of the gradient kernel's
column loop, several blocks and trips of the update kernel, the calibration's row in more than 48 KiB, 64 KiB and at 128 KiB of
dynamic LDS, the refusals above the cap and the placement loop's row chunks.  The cases and every bar live in
tests/behaviour_map_oracle.py; every comparison prints its largest error as a fraction of its bar before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import behaviour_map_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL, INT_SENTINEL = -1.2345e30, -77


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _fraction(err, bar):
    with np.errstate(all="ignore"):
        return float(np.where(err > 0, err / bar, 0.0).max()) if err.size else 0.0


def _guarded(count, cuda, dtype=torch.float64):
    """(the whole buffer, the address of its inner `count` elements): sentinel everywhere, GUARD guard words on either side."""
    t = torch.full((count + 2 * GUARD,), SENTINEL if dtype == torch.float64 else INT_SENTINEL, dtype=dtype, device=cuda)
    return t, t.data_ptr() + GUARD * t.element_size()


def _inner(t, name):
    a = t.cpu().numpy()
    fill = SENTINEL if a.dtype == np.float64 else INT_SENTINEL
    assert np.all(a[:GUARD] == fill) and np.all(a[-GUARD:] == fill), f"a guard word of {name} was written"
    return a[GUARD:-GUARD]


def _written(a, name):
    assert not np.any(a == (SENTINEL if a.dtype == np.float64 else INT_SENTINEL)), f"{name} was not written everywhere"
    return a


# ------------------------------------------------------------------------------------------------------------------ the descent
@pytest.mark.parametrize("N", bo.LARGE_SIZES)
def test_teacher_forced_step_and_cost_at_large_sizes(native_lib, cuda, N):
    """One device step from the real start and from two synthetic states: N = 1024 fills one trip of the gradient kernel's
    1024-column loop, 1025 adds a trip of one live column (and a last gradient block of one live row, a fifth update block of one
    live row), 1283 a trip of 259 columns (two of the four column groups live, three live rows in the last block)."""
    from deepfly3d_amd import ops

    P, states = bo.large_case(N)
    Pd = _dev(P, cuda)
    for k in bo.TEACHER_STAGES:
        Y, V, G = states[k]
        got = [t.cpu().numpy() for t in ops.tsne(Pd, _dev(Y, cuda), 1, first_iter=k, state=(_dev(V, cuda), _dev(G, cuda)))]
        frac, excused = bo.step_comparison(P, (Y, V, G), k, got)
        bar = bo.cost_tolerance(P, Y)
        cerr = abs(float(ops.tsne_cost(Pd, _dev(Y, cuda))) - bo.cost(P, Y))
        print(f"N = {N}, iteration {k}: Y, V, G up to {frac:.3g} of their bars, {100 * excused:.2g} % excused; the cost {cerr / bar:.3g} of its bar")
        assert frac <= 1.0 and excused <= 0.01 and cerr <= bar


@pytest.mark.parametrize("N", bo.LARGE_SIZES)
def test_joint_table_at_large_sizes(native_lib, cuda, N):
    """33 x 33 tiles at 1025 (a one-wide edge), 41 x 41 at 1283 (a three-wide one), 32 x 32 full tiles at 1024: the oracle's bits."""
    from deepfly3d_amd import ops

    cond = bo.large_cond(N)
    P = ops.joint_probabilities(_dev(cond, cuda)).cpu().numpy()
    print(f"N = {N}: |sum P - 1| = {abs(P.sum() - 1.0) / bo.EPS:.3g} x 2^-53 (bar 64)")
    assert np.array_equal(P, bo.joint(cond))
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and abs(P.sum() - 1.0) <= 64 * bo.EPS


def test_resumption_determinism_and_guard_words_at_1283(native_lib, cuda):
    """The raw df3d_tsne_run at N = 1283 on a stream of its own, Y, V, G and the workspace inside guard words: [0, 6) equals
    [0, 2) + [2, 6) bit for bit, two runs are bit-equal and equal to ops.tsne's, no guard word is touched.  Every element is
    written: after the one iteration from the start every gain is exactly 0.8 (V = 0 takes that branch), every velocity is not
    zero and every position has moved."""
    from deepfly3d_amd import ops

    lib = native_lib
    N = 1283
    P, states = bo.large_case(N)
    Y0 = states[0][0]
    need = lib.df3d_bmap_work_bytes(N)
    assert need % 16 == 0 and need >= N * 5 * 8
    side = torch.cuda.Stream(device=cuda)
    st = side.cuda_stream
    with torch.cuda.stream(side):
        Pd = _dev(P, cuda)
        runs = []
        for split in ((1,), (6,), (2, 4), (6,)):
            bufs = [_guarded(2 * N, cuda) for _ in range(3)]
            work = _guarded(need // 8, cuda)
            bufs[0][0][GUARD:-GUARD] = _dev(Y0.ravel(), cuda)
            bufs[1][0][GUARD:-GUARD] = 0.0
            bufs[2][0][GUARD:-GUARD] = 1.0
            first = 0
            for count in split:
                assert lib.df3d_tsne_run(Pd.data_ptr(), N, bufs[0][1], bufs[1][1], bufs[2][1], first, count, bo.learning_rate(N), work[1], need, st) == 0, \
                    lib.df3d_last_error()
                first += count
            side.synchronize()
            _written(_inner(work[0], "work")[: 5 * N], "work")
            runs.append([_inner(b[0], name).copy() for b, name in zip(bufs, "YVG")])
        side.synchronize()
    one, whole, halves, again = runs
    assert np.all(one[2] == 0.8) and np.all(one[1] != 0.0) and np.all(one[0] != Y0.ravel()) and np.isfinite(one[0]).all()
    for a, b, c in zip(whole, halves, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    through_ops = ops.tsne(_dev(P, cuda), _dev(Y0, cuda), 6)
    for a, t in zip(whole, through_ops):
        assert a.tobytes() == t.cpu().numpy().tobytes()
    assert np.isfinite(whole[0]).all() and whole[0].tobytes() != one[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ the wide rows
_device_calibration = {}


def _wide_on_device(lib, cuda, N, explicit):
    """(cond [5, N], beta [5], info [5]) of wide_case(N) through the raw df3d_bmap_calibrate, every output sentinel-filled inside
    guard words; kept for the tests that build on it."""
    if (N, explicit) not in _device_calibration:
        _, _, K, exclude = bo.wide_case(N)
        Kd = _dev(K, cuda)
        ex = _dev(exclude, cuda) if explicit else None
        cond, beta, info = _guarded(5 * N, cuda), _guarded(5, cuda), _guarded(5, cuda, torch.int32)
        rc = lib.df3d_bmap_calibrate(Kd.data_ptr(), 5, N, bo.PERPLEXITY, bo.ENTROPY_TOL, bo.BETA_MAX, ex.data_ptr() if explicit else None, cond[1],
                                     beta[1], info[1], torch.cuda.current_stream(cuda).cuda_stream)
        assert rc == 0, lib.df3d_last_error()
        torch.cuda.synchronize(cuda)
        _device_calibration[(N, explicit)] = tuple(_written(_inner(t[0], name), name).copy() for t, name in ((cond, "cond"), (beta, "beta"), (info, "info")))
    c, b, i = _device_calibration[(N, explicit)]
    return c.reshape(5, N), b, i


@pytest.mark.parametrize("N", bo.WIDE_SIZES)
@pytest.mark.parametrize("explicit", [False, True], ids=["none", "list"])
def test_wide_calibration(native_lib, cuda, N, explicit):
    """The row in 48 KiB of dynamic LDS (6144, the last launch that leaves the kernel's limit alone) and just above (6145), at and
    above 64 KiB (8192, the default training size, and 8193) and at the cap's 128 KiB, with no exclusion and with an explicit list."""
    from deepfly3d_amd import ops

    _, _, K, exclude = bo.wide_case(N)
    ties = bo.wide_ties(N)
    u = bo.PERPLEXITY
    cond, beta, info = _wide_on_device(native_lib, cuda, N, explicit)
    want, _, want_info = bo.calibrate(K, u, exclude if explicit else None)
    assert np.array_equal(info, want_info) and list(info) == [0, 0, 0, 0, 1]
    assert np.all((beta[:4] > 0) & (beta[:4] < bo.BETA_MAX)) and beta[4] == bo.BETA_MAX
    worst_H = worst_c = worst_s = 0.0
    for i in range(4):
        x = int(exclude[i]) if explicit else -1
        n = N - (x >= 0)
        bar_H = bo.ENTROPY_TOL + bo.entropy_rounding(n)
        H, slope, dk, keep = bo.row_entropy(K[i], beta[i], x)
        worst_H = max(worst_H, abs(H - np.log(u)) / bar_H)
        c = want[i, keep]
        worst_c = max(worst_c, _fraction(np.abs(cond[i, keep] - c), bo.conditional_tolerance(c, dk, slope, n)))
        worst_s = max(worst_s, abs(cond[i].sum() - 1.0) / ((n + 8) * bo.EPS))
        if x >= 0:
            assert cond[i, x] == 0.0
    # the tied row: beta_max, 1 / 40 on the ties and exact zeros elsewhere (the excluded column next to the last tie among them)
    tie_err = np.abs(cond[4, ties] - 1.0 / bo.WIDE_TIES).max() / (4 * bo.EPS)
    worst_s = max(worst_s, abs(cond[4].sum() - 1.0) / ((N - explicit + 8) * bo.EPS))
    print(f"N = {N}, exclude = {'list' if explicit else None}: |H(beta_device) - log u| up to {worst_H:.3g} of its bar, the conditionals up to "
          f"{worst_c:.3g} of theirs, the row sums {worst_s:.3g}, the ties {tie_err:.3g}")
    assert worst_H <= 1.0 and worst_c <= 1.0 and worst_s <= 1.0 and tie_err <= 1.0
    assert not np.delete(cond[4], ties).any()
    # the same bits through ops
    got = ops.perplexity_calibrate(_dev(K, cuda), u, _dev(exclude, cuda) if explicit else None)
    assert got[0].cpu().numpy().tobytes() == cond.tobytes() and got[1].cpu().numpy().tobytes() == beta.tobytes()
    assert got[2].dtype == torch.int32 and np.array_equal(got[2].cpu().numpy(), info)


def test_placement_at_the_cap(native_lib, cuda):
    """df3d_bmap_place on the 16 384-column conditionals of the calibration above: 64 trips of the row loop."""
    lib = native_lib
    N = bo.POINTS_CAP
    cond = _wide_on_device(lib, cuda, N, False)[0]
    Y = 10.0 * np.random.default_rng(16384).standard_normal((N, 2))
    cd, Yd, out = _dev(cond, cuda), _dev(Y, cuda), _guarded(2 * 5, cuda)
    assert lib.df3d_bmap_place(cd.data_ptr(), 5, N, Yd.data_ptr(), out[1], torch.cuda.current_stream(cuda).cuda_stream) == 0, lib.df3d_last_error()
    torch.cuda.synchronize(cuda)
    got = _written(_inner(out[0], "out"), "out").reshape(5, 2)
    frac = _fraction(np.abs(got - bo.place(cond, Y)), (N + 8) * bo.EPS * (np.abs(cond) @ np.abs(Y)))
    print(f"placement at N = {N}: up to {frac:.3g} of the bar")
    assert frac <= 1.0


def test_divergence_at_the_cap(native_lib, cuda):
    """The 4 x 16 384 table that feeds the calibration: 256 column tiles."""
    from deepfly3d_amd import ops

    pa, pb, K, _ = bo.wide_case(bo.POINTS_CAP)
    got = ops.kl_divergence(_dev(pa, cuda), _dev(pb, cuda)).cpu().numpy()
    frac = _fraction(np.abs(got - K[:4]), bo.divergence_tolerance(pa, pb))
    print(f"divergence 4 x {bo.POINTS_CAP}: up to {frac:.3g} of the bar")
    assert got.shape == (4, bo.POINTS_CAP) and np.all(got >= 0) and frac <= 1.0


def test_refusals_above_the_cap(native_lib, cuda):
    """N = 16 385 is refused by every entry that has the cap, with its message, before any buffer is touched: the buffers are
    real, small and keep their sentinels."""
    lib, err = native_lib, native_lib.df3d_last_error
    N = bo.POINTS_CAP + 1
    need = lib.df3d_bmap_work_bytes(64)
    assert lib.df3d_bmap_work_bytes(N) == 0 and need > 0
    bufs = [_guarded(64, cuda) for _ in range(5)]
    ints = _guarded(64, cuda, torch.int32)
    a, b, c, d, e = (t[1] for t in bufs)
    st = torch.cuda.current_stream(cuda).cuda_stream
    assert lib.df3d_bmap_calibrate(a, 1, N, bo.PERPLEXITY, bo.ENTROPY_TOL, bo.BETA_MAX, None, b, c, ints[1], st) == -1 and b"N must be in [1, 16384]" in err()
    assert lib.df3d_bmap_joint(a, N, b, st) == -1 and b"N must be in [0, 16384]" in err()
    assert lib.df3d_bmap_cost(a, N, b, c, d, need, st) == -1 and b"N must be in [1, 16384]" in err()
    assert lib.df3d_tsne_run(a, N, b, c, d, 0, 1, 50.0, e, need, st) == -1 and b"N must be in [1, 16384]" in err()
    torch.cuda.synchronize(cuda)
    for t, name in zip(bufs + [ints], "abcdei"):
        full = t[0].cpu().numpy()
        assert np.all(full == (SENTINEL if full.dtype == np.float64 else INT_SENTINEL)), f"buffer {name} was written by a refused call"


# ------------------------------------------------------------------------------------------------------------------ the placement loop
def test_chunked_placement_gives_the_same_bits(native_lib, cuda, monkeypatch):
    """ops.behaviour_map places the 60 frames of the planted case in one chunk; with room for 7 rows of the 120-column table per
    chunk it takes nine, the last of 4 rows.  Rows are independent: the same bits.  Two device runs are compared, so 50
    iterations are enough."""
    from deepfly3d_amd import ops

    full = bo.planted_spectra()[0]
    c = bo.PLANTED
    calls = []
    real = ops._call

    def counting(name, *args):
        if name == "df3d_bmap_place":
            calls.append(int(args[1]))
        return real(name, *args)

    monkeypatch.setattr(ops, "_call", counting)
    whole = ops.behaviour_map(_dev(full, cuda), c["perplexity"], 50, c["max_points"], seed=0)
    assert calls == [60]
    del calls[:]
    monkeypatch.setattr(ops, "_PLACE_CHUNK_BYTES", 8 * 120 * 7)
    parts = ops.behaviour_map(_dev(full, cuda), c["perplexity"], 50, c["max_points"], seed=0)
    assert calls == [7] * 8 + [4]
    for name in ("embedding", "train_index", "beta", "info"):
        assert getattr(parts, name).cpu().numpy().tobytes() == getattr(whole, name).cpu().numpy().tobytes(), name
    assert parts.kl == whole.kl and torch.isfinite(whole.embedding).all(dim=1).sum() == 180
