"""CPU tests of the behaviour map: the float64 oracle's own invariants, its independent witnesses (scipy's rel_entr,
scikit-learn's private t-SNE helpers where they import), the margins the GPU tests lean on, the C entries' refusals (no device is
touched), ops' and Core's refusals and the command-line flags."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import behaviour_map_oracle as bo  # noqa: E402


@pytest.fixture(scope="module")
def small():
    """(p [40, 25], K, cond, beta, info, P) of forty spectra, a tenth of their entries exactly zero, perplexity 6."""
    S, _ = bo.spectra(40, 25, seed=3, zeros=0.1)
    p, valid = bo.distributions(S)
    assert valid.all()
    K = bo.divergence(p, p)
    cond, beta, info = bo.calibrate(K, 6.0, "self")
    return p, K, cond, beta, info, bo.joint(cond)


# ------------------------------------------------------------------------------------------------------------------ the oracle
def test_distributions_and_validity():
    S, _ = bo.spectra(12, 7, seed=1, zeros=0.3)
    S[2] = 0.0
    S[5, 1] = np.nan
    S[7, 0] = -1e-300
    S[9, 6] = np.inf
    p, valid = bo.distributions(S.reshape(12, 7, 1))
    assert list(np.flatnonzero(~valid)) == [2, 5, 7, 9]
    assert np.all(np.isnan(p[~valid])) and np.all(p[valid] > 0)
    assert np.abs(p[valid].sum(axis=1) - 1.0).max() <= 8 * bo.EPS
    assert np.all(p[valid][S[valid] == 0] == bo.FLOOR / (1 + 7 * bo.FLOOR))   # the floor is what a silent channel gets
    for scale in (1e-6, 1e6, 2.0 ** 40):
        q = bo.distributions(S * scale)[0]
        assert np.abs(q[valid] / p[valid] - 1.0).max() <= (7 + 4) * bo.EPS


def test_divergence_matches_rel_entr(small):
    special = pytest.importorskip("scipy.special")
    p, K = small[0], small[1]
    assert np.all(K >= 0) and np.all(np.diag(K) == 0)
    want = special.rel_entr(p[:, None, :], p[None, :, :]).sum(axis=2)
    assert np.abs(K - want).max() <= 25 * 4 * bo.EPS * np.abs(np.log(p)).max()
    assert np.abs(K - K.T).max() > 1e-3   # not symmetric
    # the kernel's form e_i - P L^T agrees with the pairwise sums inside the bar the GPU test uses
    form = (p * np.log(p)).sum(axis=1)[:, None] - p @ np.log(p).T
    assert np.all(np.abs(np.maximum(form, 0) - K) <= bo.divergence_tolerance(p, p))


def test_calibration_meets_the_entropy_rule(small):
    _, K, cond, beta, info, _ = small
    assert not info.any() and np.all((beta > 0) & (beta < bo.BETA_MAX))
    assert np.abs(cond.sum(axis=1) - 1.0).max() <= 64 * bo.EPS and np.all(np.diag(cond) == 0)
    for i in range(K.shape[0]):
        H, slope, _, keep = bo.row_entropy(K[i], beta[i], i)
        assert abs(H - np.log(6.0)) <= bo.ENTROPY_TOL and slope > 0
        c = cond[i, keep]
        assert abs(-(c * np.log(c)).sum() - np.log(6.0)) <= bo.ENTROPY_TOL + bo.entropy_rounding(39)
    # no exclusion: every column takes part
    c2, b2, _ = bo.calibrate(K[:5], 6.0)
    assert np.all(c2 > 0) and np.all(np.argmax(c2, axis=1) == np.arange(5))
    for bad in (1.0, 0.5, np.nan, np.inf, 13.1):
        with pytest.raises(ValueError):
            bo.calibrate(K, bad, "self")
    bo.calibrate(K, 13.0, "self")   # 3 u = 39 = n


def test_tied_row_sets_bit_zero():
    K = np.abs(np.random.default_rng(4).standard_normal((3, 20)))
    K[1, :8] = 0.25   # eight entries tie at the minimum: perplexity 6 cannot be reached, 8 can
    K[1, 8:] += 1.0
    cond, beta, info = bo.calibrate(K, 6.0)
    assert list(info) == [0, 1, 0] and beta[1] == bo.BETA_MAX
    assert np.allclose(cond[1, :8], 1.0 / 8) and np.all(cond[1, 8:] == 0)
    assert list(bo.calibrate(K, 6.5)[2]) == [0, 1, 0]
    K[1, 6], K[1, 7] = 0.25 + 1e-9, 1.25   # six ties and a near one: 6.5 is within reach again, at a very large beta
    cond, beta, info = bo.calibrate(K, 6.5)
    assert not info.any() and 1e8 < beta[1] < bo.BETA_MAX


def test_joint_table(small):
    P = small[5]
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and abs(P.sum() - 1.0) <= 64 * bo.EPS and np.all(P >= 0)


def test_gradient_is_the_derivative_of_the_cost():
    """Central differences of the cost with step h = 1e-4: the truncation term h^2 |C'''| / 6 and the rounding term 2^-53 |C| / h
    (about 1e-12 for C near 1) meet near this step.  Measured once: 8.1e-13 at h = 1e-4 (7.8e-12 at 1e-5, 1.2e-10 at 1e-6) against
    |g| up to 7.6e-4; the bar is 1e-11."""
    P, kept = bo.teacher_case(13)
    Y = kept[399][0]
    g = bo.gradient(P, Y, 1.0)
    h, fd = 1e-4, np.zeros_like(Y)
    for i in range(13):
        for c in range(2):
            up, down = Y.copy(), Y.copy()
            up[i, c] += h
            down[i, c] -= h
            fd[i, c] = (bo.cost(P, up) - bo.cost(P, down)) / (2 * h)
    print(f"finite difference: {np.abs(fd - g).max():.3g} against |g| up to {np.abs(g).max():.3g}")
    assert np.abs(fd - g).max() <= 1e-11 and np.abs(g).max() > 1e-4


def test_training_index_rule():
    for Tv, cap in ((5, 8), (8, 8), (13, 8), (180, 120), (100000, 8192)):
        rows = bo.train_rows(Tv, cap)
        N = min(Tv, cap)
        assert len(rows) == N and rows[0] == 0 and rows[-1] == ((N - 1) * Tv) // N < Tv and np.all(np.diff(rows) >= 1)
        assert np.array_equal(rows, np.floor(np.arange(N) * Tv / N).astype(np.int64))
    assert np.array_equal(bo.train_rows(5, 8), np.arange(5)) and np.array_equal(bo.train_rows(12, 8), [0, 1, 3, 4, 6, 7, 9, 10])


def test_planted_behaviours_separate_and_invalid_rows_are_nan():
    full, lab, res, kls = bo.planted_case()
    emb = res["embedding"]
    assert np.array_equal(np.isnan(emb).any(axis=1), lab < 0) and np.array_equal(np.isnan(emb[:, 0]), np.isnan(emb[:, 1]))
    assert np.array_equal(np.isnan(res["beta"]), lab < 0) and not res["info"].any()
    assert len(res["train_index"]) == 120 and np.all(lab[res["train_index"]] >= 0)
    assert sorted(set(lab[res["train_index"]])) == [0, 1, 2]          # every behaviour trains
    placed = np.setdiff1d(np.flatnonzero(lab >= 0), res["train_index"])
    assert len(placed) == 60 and sorted(set(lab[placed])) == [0, 1, 2]   # and every behaviour has placed frames
    own_label, between, own = bo.separation(emb, lab)
    print(f"planted: between-label {between:.3g}, own-label nearest neighbour up to {own:.3g}; KL {res['kl']:.4f}, perturbed "
          f"{kls.min():.4f} .. {kls.max():.4f}")
    assert own_label and between >= 2 * own
    assert np.ptp(kls) > 0


def test_teacher_seeds_keep_the_excused_components_under_one_percent():
    """The GPU test excuses a gain component whose g V lies within the gradient's bar of zero.  On the oracle's own states the
    fraction is far below the 1 % cap (measured: none at all), and the oracle's own step sits inside its bars."""
    for N in bo.TEACHER_SIZES:
        P, kept = bo.teacher_case(N)
        assert sorted(kept) == list(bo.TEACHER_STAGES)
        assert np.abs(kept[0][0]).max() < 1e-3 and not kept[0][1].any()
        for k, state in kept.items():
            Yn, Vn, Gn, _ = bo.step(P, *state, k)
            frac, excused = bo.step_comparison(P, state, k, (Yn, Vn, Gn))
            assert frac == 0.0 and excused <= 0.01, (N, k, excused)


@pytest.mark.parametrize("N", bo.LARGE_SIZES)
def test_large_cases_stay_inside_their_bars_in_another_summation_order(N):
    """What the GPU step tests at LARGE_SIZES rest on.  The oracle's step with every point renumbered back to front sums each
    row's columns, and Z, in the opposite order: a stand-in for the device's order.  It stays inside step_comparison's bars with
    at most 1 % of the components excused (the existing cap, not a measurement), at the real start and at both synthetic
    states, and the synthetic gains take both branches and the floor."""
    P, states = bo.large_case(N)
    assert sorted(states) == list(bo.TEACHER_STAGES) and P.shape == (N, N)
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and abs(P.sum() - 1.0) <= 64 * bo.EPS
    assert np.abs(states[0][0]).max() < 1e-3 and not states[0][1].any() and np.all(states[0][2] == 1.0)
    Pr = np.ascontiguousarray(P[::-1, ::-1])
    for k, state in states.items():
        got = [a[::-1] for a in bo.step(Pr, *(a[::-1] for a in state), k)[:3]]
        frac, excused = bo.step_comparison(P, state, k, got)
        print(f"N = {N}, stage {k}: the reversed order is {frac:.3g} of the bars from the oracle, {100 * excused:.2g} % excused")
        assert frac <= 1.0 and excused <= 0.01, (N, k, frac, excused)
        if k:
            Y, V, G = state
            g = bo.gradient(P, Y, bo.schedule(k)[0])
            up = g * V < 0.0
            assert set(np.unique(G)) == set(bo.GAINS)
            assert up.any() and (~up).any()                                      # G + 0.2 and 0.8 G
            assert (~up & (G == 0.01)).any() and (up & (G == 0.01)).any()         # 0.008 is lifted to the floor, 0.21 is not
            assert np.abs(Y).max() > 1.0 and V.all()


@pytest.mark.parametrize("N", bo.WIDE_SIZES)
def test_wide_cases_calibrate_and_their_tied_row_is_refused(N):
    """What the GPU calibration tests at WIDE_SIZES rest on: the oracle's own beta meets the entropy bar on the four ordinary
    rows with and without an exclusion, and the tied row gets beta_max, bit 0 and 1 / 40 on its ties.  Nothing O(N^2) is built."""
    pa, pb, K, exclude = bo.wide_case(N)
    ties = bo.wide_ties(N)
    assert K.shape == (5, N) and pa.shape == (4, 25) and pb.shape == (N, 25) and list(exclude[:4]) == [N - 1, -1, 0, 4097]
    assert N - 2 in ties and exclude[4] not in ties and np.all(K[4, ties] == K[4].min()) and np.delete(K[4], ties).min() >= K[4].min() + 0.75
    for ex in (None, exclude):
        cond, beta, info = bo.calibrate(K, bo.PERPLEXITY, ex)
        assert list(info) == [0, 0, 0, 0, 1] and beta[4] == bo.BETA_MAX and np.all((beta[:4] > 1.0) & (beta[:4] < 1e3))
        for i in range(4):
            x = -1 if ex is None else int(ex[i])
            n = N - (x >= 0)
            H, slope, _, keep = bo.row_entropy(K[i], beta[i], x)
            assert abs(H - np.log(bo.PERPLEXITY)) <= bo.ENTROPY_TOL + bo.entropy_rounding(n) and slope > 0
            assert keep.sum() == n and (x < 0 or cond[i, x] == 0.0) and abs(cond[i].sum() - 1.0) <= (n + 8) * bo.EPS
        assert np.array_equal(cond[4, ties], np.full(bo.WIDE_TIES, 1.0 / bo.WIDE_TIES)) and not np.delete(cond[4], ties).any()


def test_resumed_runs_are_the_whole_run():
    P, _ = bo.teacher_case(13)
    Y0 = bo.initial(13, 5)
    whole = bo.run(P, Y0, 260)
    first = bo.run(P, Y0, 240)
    second = bo.run(P, first[0], 20, first_iter=240, state=first[1:])
    assert all(np.array_equal(a, b) for a, b in zip(whole, second))


# ------------------------------------------------------------------------------------------------------------------ the witness
def test_scikit_learn_witness_of_cost_gradient_and_joint_table(small):
    """scikit-learn's private helpers as an independent witness, at THEIR precision: _kl_divergence clips P and Q at machine epsilon
    (harmless here), _joint_probabilities searches beta in float32 for 100 steps to 1e-5 in the entropy."""
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    distance = pytest.importorskip("scipy.spatial.distance")
    if not (hasattr(tsne, "_kl_divergence") and hasattr(tsne, "_joint_probabilities")):
        pytest.skip("this scikit-learn has no _kl_divergence / _joint_probabilities")
    _, K, _, _, _, P = small
    N = P.shape[0]
    Y = np.random.default_rng(8).standard_normal((N, 2))
    kl, grad = tsne._kl_divergence(Y.ravel(), distance.squareform(P, checks=False), 1.0, N, 2)
    assert abs(kl - bo.cost(P, Y)) <= 1e-12 * max(1.0, abs(kl))
    assert np.abs(grad.reshape(N, 2) - bo.gradient(P, Y, 1.0)).max() <= 1e-12 * np.abs(grad).max()
    # the joint table needs a symmetric input there (it reads the upper triangle's conditional from both): use K + K^T
    sym = K + K.T
    Pw = distance.squareform(tsne._joint_probabilities(sym.astype(np.float32), 6.0, 0))
    Po = bo.joint(bo.calibrate(sym, 6.0, "self")[0])
    print(f"joint table against scikit-learn: {np.abs(Pw - Po).max():.3g} of entries up to {Po.max():.3g}")
    assert np.abs(Pw - Po).max() <= 1e-4 * Po.max()


# ------------------------------------------------------------------------------------------------------------------ the C entries
def test_entries_validate_arguments_without_gpu(native_lib):
    lib, err = native_lib, native_lib.df3d_last_error
    base = 1 << 28
    buf = [ctypes.c_void_p(base + k * (1 << 24)) for k in range(8)]
    at = lambda k, off=0: ctypes.c_void_p(buf[k].value + off)   # noqa: E731
    tol, bmax = bo.ENTROPY_TOL, bo.BETA_MAX

    assert lib.df3d_bmap_work_bytes(0) == 0 and lib.df3d_bmap_work_bytes(16385) == 0
    assert lib.df3d_bmap_work_bytes(13) >= 13 * 5 * 8 and lib.df3d_bmap_work_bytes(16384) % 16 == 0

    def prepare(S=buf[0], T=8, D=25, floor=1e-9, p=buf[1], logp=buf[2], e=buf[3], valid=buf[4]):
        return lib.df3d_bmap_prepare(S, T, D, floor, p, logp, e, valid, None)

    assert lib.df3d_bmap_prepare(None, 0, 25, 1e-9, None, None, None, None, None) == 0   # empty: nothing to do
    assert prepare(T=-1) == -1 and b"T must be >= 0" in err()
    assert prepare(D=0) == -1 and b"D must be >= 1" in err()
    for bad in (-1e-9, np.nan, np.inf):
        assert prepare(floor=bad) == -1 and b"floor" in err()
    assert prepare(T=1 << 40) == -1 and b"too large" in err()
    for name in ("S", "p", "logp", "e", "valid"):
        assert prepare(**{name: None}) == -1 and b"null pointer: " + name.encode() in err()
    assert prepare(p=at(1, 4)) == -1 and b"p must be 8-byte aligned" in err()
    assert prepare(valid=at(4, 2)) == -1 and b"valid must be 4-byte aligned" in err()
    assert prepare(p=at(0, 8 * 25 * 8 - 8)) == -1 and b"p must not overlap S" in err()
    assert prepare(logp=at(1)) == -1 and b"logp must not overlap p" in err()
    assert lib.df3d_bmap_logs(buf[0], 4, 0, buf[1], buf[2], None) == -1 and b"D must be" in err()
    assert lib.df3d_bmap_logs(buf[0], 4, 3, buf[0], buf[2], None) == -1 and b"logp must not overlap p" in err()

    def divergence(pa=buf[0], ea=buf[1], M=8, lb=buf[2], N=9, D=25, K=buf[3]):
        return lib.df3d_bmap_divergence(pa, ea, M, lb, N, D, K, None)

    assert lib.df3d_bmap_divergence(None, None, 0, None, 9, 25, None, None) == 0
    assert divergence(M=-1) == -1 and b"M must be" in err()
    assert divergence(N=-2) == -1 and b"N must be" in err()
    assert divergence(D=0) == -1 and b"D must be" in err()
    assert divergence(M=65535 * 128 + 1) == -1 and b"row chunks" in err()
    assert divergence(N=1 << 50) == -1 and b"N is too large" in err()
    for name in ("pa", "ea", "lb", "K"):
        assert divergence(**{name: None}) == -1 and b"null pointer: " + name.encode() in err()
    assert divergence(K=at(3, 4)) == -1 and b"K must be 8-byte aligned" in err()
    assert divergence(K=at(0, 8)) == -1 and b"K must not overlap pa" in err()
    assert divergence(K=at(2, 8)) == -1 and b"K must not overlap lb" in err()

    def calibrate(K=buf[0], M=40, N=40, u=6.0, tol=tol, bmax=bmax, exclude=buf[1], cond=buf[2], beta=buf[3], info=buf[4]):
        return lib.df3d_bmap_calibrate(K, M, N, u, tol, bmax, exclude, cond, beta, info, None)

    assert lib.df3d_bmap_calibrate(None, 0, 40, 6.0, tol, bmax, None, None, None, None, None) == 0
    assert calibrate(M=-1) == -1 and b"M must be" in err()
    for N in (0, 16385):
        assert calibrate(N=N) == -1 and b"N must be in [1, 16384]" in err()
    for bad in (1.0, 0.0, -3.0, np.nan, np.inf):
        assert calibrate(u=bad) == -1 and b"perplexity must be finite and > 1" in err(), bad
    assert calibrate(u=13.1) == -1 and b"smallest frame count accepted is 41" in err() and b"largest perplexity for this one 13" in err()
    assert calibrate(N=95, exclude=None, u=32.0) == -1 and b"smallest frame count accepted is 96" in err()
    assert calibrate(N=96, u=32.0) == -1 and b"smallest frame count accepted is 97" in err() and b"31.66" in err()
    assert calibrate(tol=0.0) == -1 and b"tol" in err()
    assert calibrate(bmax=np.inf) == -1 and b"beta_max" in err()
    for name in ("K", "cond", "beta", "info"):
        assert calibrate(**{name: None}) == -1 and b"null pointer: " + name.encode() in err()
    assert calibrate(cond=at(0, 16)) == -1 and b"cond must not overlap K" in err()
    assert calibrate(exclude=at(1, 2)) == -1 and b"exclude must be 4-byte aligned" in err()
    assert calibrate(info=at(3)) == -1 and b"info must not overlap beta" in err()

    assert lib.df3d_bmap_joint(None, 0, None, None) == 0
    assert lib.df3d_bmap_joint(buf[0], -1, buf[1], None) == -1 and b"N must be" in err()
    assert lib.df3d_bmap_joint(buf[0], 40, None, None) == -1 and b"null pointer: P" in err()
    assert lib.df3d_bmap_joint(buf[0], 40, at(0, 40 * 40 * 8 - 8), None) == -1 and b"P must not overlap cond" in err()

    assert lib.df3d_bmap_place(None, 0, 40, None, None, None) == 0
    assert lib.df3d_bmap_place(buf[0], 5, 0, buf[1], buf[2], None) == -1 and b"N must be" in err()
    assert lib.df3d_bmap_place(buf[0], 5, 40, at(1, 8), buf[2], None) == -1 and b"Y must be 16-byte aligned" in err()
    assert lib.df3d_bmap_place(buf[0], 5, 40, buf[1], None, None) == -1 and b"null pointer: out" in err()
    assert lib.df3d_bmap_place(buf[0], 5, 40, buf[1], at(1, 16), None) == -1 and b"out must not overlap Y" in err()

    need = lib.df3d_bmap_work_bytes(40)

    def run(P=buf[0], N=40, Y=buf[1], V=buf[2], G=buf[3], first=0, num=5, lr=50.0, work=buf[4], work_len=need):
        return lib.df3d_tsne_run(P, N, Y, V, G, first, num, lr, work, work_len, None)

    assert lib.df3d_tsne_run(None, 40, None, None, None, 7, 0, 50.0, None, 0, None) == 0   # no iterations: nothing to do
    for N in (0, 16385):
        assert run(N=N) == -1 and b"N must be in [1, 16384]" in err()
    assert run(first=-1) == -1 and b"first_iter" in err()
    assert run(num=-1) == -1 and b"num_iters" in err()
    assert run(first=2 ** 31 - 3, num=5) == -1 and b"num_iters" in err()
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert run(lr=bad) == -1 and b"lr must be finite and > 0" in err()
    assert run(work_len=need - 1) == -1 and b"work buffer too small (df3d_bmap_work_bytes)" in err()
    for name in ("P", "Y", "V", "G", "work"):
        assert run(**{name: None}) == -1 and b"null pointer: " + name.encode() in err()
    assert run(Y=at(1, 8)) == -1 and b"Y must be 16-byte aligned" in err()
    assert run(work=at(4, 8)) == -1 and b"work must be 16-byte aligned" in err()
    assert run(V=at(1, 16)) == -1 and b"V must not overlap Y" in err()
    assert run(work=at(0, 40 * 40 * 8 - 16)) == -1 and b"work must not overlap P" in err()

    def cost(P=buf[0], N=40, Y=buf[1], out=buf[2], work=buf[4], work_len=need):
        return lib.df3d_bmap_cost(P, N, Y, out, work, work_len, None)

    assert cost(N=0) == -1 and b"N must be" in err()
    assert cost(work_len=8) == -1 and b"work buffer too small" in err()
    assert cost(out=None) == -1 and b"null pointer: cost" in err()
    assert cost(out=at(1)) == -1 and b"cost must not overlap Y" in err()


# ------------------------------------------------------------------------------------------------------------------ ops, config, CLI, Core
def test_config_matches_the_oracle():
    from deepfly3d_amd import config as cfg

    assert (cfg.BEHAVIOUR_FLOOR, cfg.BEHAVIOUR_MAX_POINTS, cfg.BEHAVIOUR_POINTS_CAP) == (bo.FLOOR, bo.MAX_POINTS, bo.POINTS_CAP) == (1e-9, 8192, 16384)
    assert (cfg.BEHAVIOUR_PERPLEXITY, cfg.BEHAVIOUR_ENTROPY_TOL, cfg.BEHAVIOUR_BETA_MAX) == (bo.PERPLEXITY, bo.ENTROPY_TOL, bo.BETA_MAX) == (32, 1e-10, 1e12)
    assert (cfg.BEHAVIOUR_ITERATIONS, cfg.BEHAVIOUR_EXAGGERATION_ITERATIONS) == (bo.ITERATIONS, bo.EXAGGERATION_ITERATIONS) == (1000, 250)


def test_ops_points_rule_and_refusals(native_lib):
    import torch

    from deepfly3d_amd import ops

    assert ops.behaviour_map_points(100000) == (8192, 32.0) and ops.behaviour_map_points(97) == (97, 32.0)
    assert ops.behaviour_map_points(15, 4) == (15, 4.0) and ops.behaviour_map_points(13, 4.0) == (13, 4.0)
    assert ops.behaviour_map_points(500, 10, 120) == (120, 10.0)
    with pytest.raises(ValueError, match=r"perplexity 32 needs at least 97 frames .* this recording has 15 valid frames: the largest perplexity "
                                         r"accepted for 15 frames is 4\.667"):
        ops.behaviour_map_points(15)
    with pytest.raises(ValueError, match="needs at least 14 frames"):
        ops.behaviour_map_points(13, 4.2)
    with pytest.raises(ValueError, match="max_points is 90"):
        ops.behaviour_map_points(1000, None, 90)
    for bad in (0, 16385, -4):
        with pytest.raises(ValueError, match=r"max_points must be in \[1, 16384\]"):
            ops.behaviour_map_points(1000, None, bad)
    for bad in (1.0, np.nan, np.inf, -2.0):
        with pytest.raises(ValueError, match="perplexity must be finite and > 1"):
            ops.behaviour_map_points(1000, bad)
    for Tv, N in ((5, 5), (13, 8), (180, 120)):
        assert np.array_equal(ops.behaviour_train_rows(Tv, N), bo.train_rows(Tv, N))
    x = torch.zeros((200, 6), dtype=torch.float64)   # on the host: refused
    with pytest.raises(ValueError, match="S must be"):
        ops.spectrogram_distributions(x)
    with pytest.raises(ValueError, match="needs at least 97 frames"):
        ops.behaviour_map(x[:50])   # before the device is asked for
    with pytest.raises(ValueError, match="S must be"):
        ops.behaviour_map(x)
    for fn in (ops.kl_divergence, ops.tsne, ops.tsne_cost):
        with pytest.raises(ValueError, match="CUDA tensor"):
            fn(x, x)
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.perplexity_calibrate(x)


def test_cli_flags_parse_and_count_as_something_to_do(tmp_path, monkeypatch, capsys):
    from deepfly3d_amd import cli

    args = cli.parse_cli_args(["/tmp/x", "--behaviour-map"])
    assert args.behaviour_map is True and args.behaviour_perplexity is None and not args.angle_spectrogram
    assert cli.parse_cli_args(["/tmp/x"]).behaviour_map is False
    args = cli.parse_cli_args(["/tmp/x", "--behaviour-map", "--behaviour-perplexity", "4", "--rigid-legs", "--skip-pose-estimation"])
    assert args.behaviour_map and args.behaviour_perplexity == 4.0 and args.rigid_legs and args.skip_estimation
    for argv, what in ((["--behaviour-perplexity", "4"], "needs --behaviour-map"), (["--behaviour-map", "--behaviour-perplexity", "1"], "finite and > 1"),
                       (["--behaviour-map", "--behaviour-perplexity", "nan"], "finite and > 1")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(["/tmp/x"] + argv)
        assert what in capsys.readouterr().err

    class Reached(Exception):
        pass

    def core(*a, **kw):
        raise Reached()

    monkeypatch.setattr(cli, "Core", core)
    assert cli.run(cli.parse_cli_args([str(tmp_path), "--skip-pose-estimation"])) == 0
    with pytest.raises(Reached):
        cli.run(cli.parse_cli_args([str(tmp_path), "--skip-pose-estimation", "--behaviour-map"]))


def test_cli_refuses_before_any_work(tmp_path, golden_dir, monkeypatch):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    folder = tmp_path / "images"   # one frame per camera and no earlier result
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    config.pop("image_shape", None)
    with pytest.raises(RuntimeError, match="--behaviour-map needs calibrated cameras"):
        cli.run(cli.parse_cli_args([str(folder), "--behaviour-map", "--skip-pose-estimation"]))
    # a recording of one frame is too short for any perplexity: refused before the pose estimation starts
    monkeypatch.setattr(Core, "pose2d_estimation", lambda *a, **kw: pytest.fail("work was started"))
    with pytest.raises(ValueError, match="perplexity 32 needs at least 97 frames .* this recording has 1 valid frames"):
        cli.run(cli.parse_cli_args([str(folder), "--behaviour-map"]))
    config.pop("image_shape", None)
    assert not [f for f in os.listdir(str(folder) + "_df3d") if f.startswith("df3d_result")]


class _Net:
    def __init__(self, calibrated):
        self.calibrated, self.points3d = calibrated, None

    def has_calibration(self):
        return self.calibrated


def _bare_core():
    from deepfly3d_amd.core import Core

    core = Core.__new__(Core)
    core.camNet, core.device, core.is_primary, core.num_images = _Net(False), "cpu", True, 15
    core.get_fps = lambda: None
    return core


def test_core_behaviour_map_refusals(monkeypatch):
    from deepfly3d_amd import distributed as dd

    core = _bare_core()
    for net in (_Net(False), None):
        core.camNet = net
        with pytest.raises(RuntimeError, match=r"behaviour_map needs calibrated cameras: run calibrate_calc\(\)"):
            core.behaviour_map(perplexity=4)
    core.camNet = _Net(True)
    with pytest.raises(ValueError, match="perplexity 32 needs at least 97 frames .* has 15 valid frames"):
        core.behaviour_map()
    with pytest.raises(TypeError, match="behaviour_map got unexpected bank arguments .*window"):
        core.behaviour_map(perplexity=4, window=3)
    with pytest.raises(ValueError, match="max_points"):
        core.behaviour_map(perplexity=4, max_points=20000)
    monkeypatch.setattr(dd, "current", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="behaviour_map is a rank-0"):
        core.behaviour_map(perplexity=4)


def test_result_written_without_the_flag_is_unchanged(tmp_path):
    core = _bare_core()
    core.camNet = None
    core.points2d = np.arange(7 * 3 * 19 * 2, dtype=np.float64).reshape(7, 3, 19, 2)
    core.points2d_argmax, core.camera_ordering, core.conf = None, np.arange(7), np.ones((7, 3, 19))
    (tmp_path / "in").mkdir()
    core.output_folder, core.input_folder = str(tmp_path), str(tmp_path / "in")
    core._write_result()
    with open(core.save_path, "rb") as f:
        plain = f.read()
    assert list(pickle.loads(plain).keys()) == ["points2d", "camera_ordering", "heatmap_confidence"]
    core._write_result(None, False, False, False, False, None)
    with open(core.save_path, "rb") as f:
        assert f.read() == plain
    os.remove(core.save_path)
    with pytest.raises(ValueError, match="needs at least 97 frames"):   # 15 frames, the default perplexity: before anything is written
        core._write_result(behaviour_map=True)
    with pytest.raises(RuntimeError, match="behaviour_map needs calibrated cameras"):
        core._write_result(behaviour_map=True, behaviour_perplexity=4.0)
    assert not os.path.exists(core.save_path)
