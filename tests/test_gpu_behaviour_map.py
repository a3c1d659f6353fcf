"""GPU tests of the behaviour map: csrc/behaviour_map.hip against the float64 oracle of
tests/behaviour_map_oracle.py, stage by stage.  Every bar is derived there, next to the sum it bounds, and every comparison prints
its largest error as a fraction of its bar before it asserts."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import behaviour_map_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _fraction(err, bar):
    with np.errstate(all="ignore"):
        return float(np.where(err > 0, err / bar, 0.0).max()) if err.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ distributions
def test_distributions_validity_floor_and_scale(native_lib, cuda):
    from deepfly3d_amd import ops

    S, _ = bo.spectra(70, 25, seed=2, zeros=0.3)
    S[3] = 0.0
    S[17, 4] = np.nan
    S[40, 0] = -1e-300
    S[69, 24] = np.inf
    want, valid = bo.distributions(S)
    assert (S[valid] == 0).any()
    for scale in (1.0, 1e-6, 1e6):
        p, v = ops.spectrogram_distributions(_dev(S * scale, cuda))
        p, v = p.cpu().numpy(), v.cpu().numpy()
        assert v.dtype == np.bool_ and np.array_equal(v, valid) and np.all(np.isnan(p[~valid])) and np.all(p[valid] > 0)
        rel = np.abs(p[valid] / want[valid] - 1.0).max()
        print(f"scale {scale:g}: the distributions differ from the oracle's by {rel / bo.EPS:.3g} x 2^-53 (bar {25 + 4})")
        assert rel <= (25 + 4) * bo.EPS   # a D-term sum in another order, a quotient, a sum and a product
    # one wide row (several strides of the block) and a single channel
    for T, D in ((3, 1200), (5, 1)):
        S, _ = bo.spectra(T, D, seed=D, zeros=0.2 if D > 1 else 0.0)
        p, v = ops.spectrogram_distributions(_dev(S, cuda))
        assert v.all() and np.abs(p.cpu().numpy() / bo.distributions(S)[0] - 1.0).max() <= (D + 4) * bo.EPS


# ------------------------------------------------------------------------------------------------------------------ divergence
@pytest.mark.parametrize("M,N,D", [(1, 13, 1), (13, 1, 3), (63, 64, 25), (64, 65, 25), (65, 129, 3), (129, 63, 25), (129, 13, 1), (13, 65, 1200)])
def test_divergence(native_lib, cuda, M, N, D):
    """Tile edges (128 x 64 tiles, chunks of 16 along D), exact zeros under the floor, duplicate rows."""
    from deepfly3d_amd import ops

    Sa, _ = bo.spectra(M, D, seed=10 * M + D, zeros=0.25 if D > 1 else 0.0)
    Sb, _ = bo.spectra(N, D, seed=10 * N + D + 1, zeros=0.25 if D > 1 else 0.0)
    Sb[N // 2] = Sa[0]            # a duplicate across the sets
    if M > 1:
        Sa[M - 1] = Sa[0]         # and inside one
    pa, pb = bo.distributions(Sa)[0], bo.distributions(Sb)[0]
    got = ops.kl_divergence(_dev(pa, cuda), _dev(pb, cuda)).cpu().numpy()
    want, bar = bo.divergence(pa, pb), bo.divergence_tolerance(pa, pb)
    assert got.shape == (M, N) and np.all(got >= 0)
    err = np.abs(got - want)
    print(f"M, N, D = {M}, {N}, {D}: max |device - oracle| = {err.max():.3g}, {_fraction(err, bar):.3g} of the bar")
    assert np.all(err <= bar)
    assert got[0, N // 2] <= bar[0, N // 2] and np.array_equal(got[0], got[M - 1])
    if D > 1:
        assert want.max() > 1e-2   # the floor at work: a silent channel costs log(p / floor), not infinity


# ------------------------------------------------------------------------------------------------------------------ calibration
def _square_table(N, seed=0):
    S, _ = bo.spectra(N, 25, seed=300 + N + seed)
    p = bo.distributions(S)[0]
    return bo.divergence(p, p)


@pytest.mark.parametrize("N", [13, 64, 65, 257])
@pytest.mark.parametrize("exclude", ["self", None])
def test_calibration(native_lib, cuda, N, exclude):
    from deepfly3d_amd import ops

    K = _square_table(N)
    u = 4.0 if N == 13 else 10.0
    cond, beta, info = (t.cpu().numpy() for t in ops.perplexity_calibrate(_dev(K, cuda), u, exclude))
    want = bo.calibrate(K, u, exclude)[0]
    n = N - (exclude is not None)
    bar_H = bo.ENTROPY_TOL + bo.entropy_rounding(n)
    assert not info.any() and np.all((beta > 0) & (beta < bo.BETA_MAX))
    worst_H = worst_c = 0.0
    for i in range(N):
        H, slope, dk, keep = bo.row_entropy(K[i], beta[i], i if exclude else -1)
        worst_H = max(worst_H, abs(H - np.log(u)) / bar_H)
        c = want[i, keep]
        bar_c = bo.conditional_tolerance(c, dk, slope, n)
        worst_c = max(worst_c, _fraction(np.abs(cond[i, keep] - c), bar_c))
        if exclude:
            assert cond[i, i] == 0.0
    print(f"N = {N}, exclude = {exclude}: |H(beta_device) - log u| up to {worst_H:.3g} of its bar ({bar_H:.3g}), the conditionals up to {worst_c:.3g} of theirs")
    assert worst_H <= 1.0 and worst_c <= 1.0
    assert np.abs(cond.sum(axis=1) - 1.0).max() <= (n + 8) * bo.EPS


def test_calibration_ties_and_refusals(native_lib, cuda):
    from deepfly3d_amd import ops

    K = np.abs(np.random.default_rng(4).standard_normal((3, 20)))
    K[1, :8] = 0.25
    K[1, 8:] += 1.0
    cond, beta, info = (t.cpu().numpy() for t in ops.perplexity_calibrate(_dev(K, cuda), 6.0))
    assert list(info) == [0, 1, 0] and beta[1] == bo.BETA_MAX
    assert np.abs(cond[1, :8] - 0.125).max() <= 4 * bo.EPS and np.all(cond[1, 8:] == 0)
    want = bo.calibrate(K, 6.0)
    assert np.abs(cond[[0, 2]] - want[0][[0, 2]]).max() <= 1e-8
    K[1, 6], K[1, 7] = 0.25 + 1e-9, 1.25   # six ties and a near one: perplexity 6.5 is met at a beta of about 1e9
    _, beta, info = ops.perplexity_calibrate(_dev(K, cuda), 6.5)
    assert not info.cpu().numpy().any() and 1e8 < float(beta[1]) < bo.BETA_MAX
    assert abs(bo.row_entropy(K[1], float(beta[1]))[0] - np.log(6.5)) <= bo.ENTROPY_TOL + bo.entropy_rounding(20)
    Kd = _dev(K, cuda)
    with pytest.raises(ValueError, match=r"perplexity 7 needs at least 21 points .* smallest frame count accepted is 21, the largest perplexity for this one 6\.66"):
        ops.perplexity_calibrate(Kd, 7.0)
    with pytest.raises(ValueError, match="perplexity must be finite and > 1"):
        ops.perplexity_calibrate(Kd, 1.0)
    with pytest.raises(ValueError, match="exclude"):
        ops.perplexity_calibrate(Kd, 4.0, "self")   # not square
    sq = _dev(_square_table(13), cuda)
    with pytest.raises(ValueError, match="smallest frame count accepted is 14"):
        ops.perplexity_calibrate(sq, 4.2, "self")
    # an explicit exclusion list, -1 for none
    ex = torch.tensor([2, -1, 0] + [-1] * 10, dtype=torch.int32, device=cuda)
    c = ops.perplexity_calibrate(sq, 4.0, ex)[0].cpu().numpy()
    assert c[0, 2] == 0 and c[2, 0] == 0 and np.all(c[1] > 0) and np.abs(c - bo.calibrate(sq.cpu().numpy(), 4.0, ex.cpu().numpy())[0]).max() <= 1e-8
    P = ops.joint_probabilities(ops.perplexity_calibrate(sq, 4.0, "self")[0]).cpu().numpy()
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and abs(P.sum() - 1.0) <= 64 * bo.EPS


# ------------------------------------------------------------------------------------------------------------------ the descent
@pytest.mark.parametrize("N", bo.TEACHER_SIZES)
def test_teacher_forced_step_and_cost(native_lib, cuda, N):
    """One device step from the oracle's state at the start (all distances about 1e-4), in mid-exaggeration and at the end."""
    from deepfly3d_amd import ops

    P, kept = bo.teacher_case(N)
    Pd = _dev(P, cuda)
    for k in bo.TEACHER_STAGES:
        Y, V, G = kept[k]
        got = [t.cpu().numpy() for t in ops.tsne(Pd, _dev(Y, cuda), 1, first_iter=k, state=(_dev(V, cuda), _dev(G, cuda)))]
        frac, excused = bo.step_comparison(P, (Y, V, G), k, got)
        bar = bo.cost_tolerance(P, Y)   # the cost at the same state
        cerr = abs(float(ops.tsne_cost(Pd, _dev(Y, cuda))) - bo.cost(P, Y))
        print(f"N = {N}, iteration {k}: Y, V, G up to {frac:.3g} of their bars, {100 * excused:.2g} % excused; the cost {cerr / bar:.3g} of its bar")
        assert frac <= 1.0 and excused <= 0.01 and cerr <= bar


def test_resumption_determinism_guard_words_and_a_side_stream(native_lib, cuda):
    """The raw entries on sentinel-filled buffers inside guard words, on a stream of their own: [0, 30) equals [0, 12) + [12, 30) bit for
    bit, two runs are bit-equal, every output element is written and nothing outside is."""
    lib = native_lib
    N, M, D, GUARD = 65, 13, 25, 64
    sentinel = -1.2345e30
    P, _ = bo.teacher_case(N)
    Sa, _ = bo.spectra(M, D, seed=5, zeros=0.2)
    Sb, _ = bo.spectra(N, D, seed=6)
    need = lib.df3d_bmap_work_bytes(N)
    assert need % 16 == 0 and need >= N * 5 * 8
    side = torch.cuda.Stream(device=cuda)
    st = side.cuda_stream

    def guarded(count, dtype=torch.float64):
        t = torch.full((count + 2 * GUARD,), sentinel if dtype == torch.float64 else -77, dtype=dtype, device=cuda)
        return t, t.data_ptr() + GUARD * t.element_size()

    def inner(t):
        a = t.cpu().numpy()
        fill = sentinel if a.dtype == np.float64 else -77
        assert np.all(a[:GUARD] == fill) and np.all(a[-GUARD:] == fill), "a guard word was written"
        return a[GUARD:-GUARD]

    with torch.cuda.stream(side):
        Pd, Y0 = _dev(P, cuda), bo.initial(N, 1)
        runs = []
        for split in ((30,), (12, 18), (30,)):
            bufs = [guarded(2 * N) for _ in range(3)]
            work = guarded(need // 8)
            bufs[0][0][GUARD:-GUARD] = _dev(Y0.ravel(), cuda)
            bufs[1][0][GUARD:-GUARD] = 0.0
            bufs[2][0][GUARD:-GUARD] = 1.0
            first = 0
            for count in split:
                assert lib.df3d_tsne_run(Pd.data_ptr(), N, bufs[0][1], bufs[1][1], bufs[2][1], first, count, bo.learning_rate(N), work[1], need, st) == 0, \
                    lib.df3d_last_error()
                first += count
            side.synchronize()
            inner(work[0])
            runs.append([inner(b[0]).copy() for b in bufs])
        for a, b, c in zip(*runs):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        want = bo.run(P, Y0, 30)
        # 30 free-running iterations amplify rounding (see the trajectory test): only a loose sanity bar here
        assert np.abs(runs[0][0].reshape(N, 2) - want[0]).max() <= 1e-4 * np.abs(want[0]).max()

        # prepare -> divergence -> calibrate -> place, and joint and cost on the training table: every element written, no guard touched
        Sd, Td = _dev(Sa, cuda), _dev(Sb, cuda)
        pa, la, ea, va = guarded(M * D), guarded(M * D), guarded(M), guarded(M, torch.int32)
        pb, lb, eb, vb = guarded(N * D), guarded(N * D), guarded(N), guarded(N, torch.int32)
        Kt, ct, bt, it, out = guarded(M * N), guarded(M * N), guarded(M), guarded(M, torch.int32), guarded(2 * M)
        Pj, cost, work = guarded(N * N), guarded(1), guarded(need // 8)
        Yd = _dev(want[0], cuda)
        cd = _dev(bo.calibrate(bo.divergence(bo.distributions(Sb)[0], bo.distributions(Sb)[0]), 10.0, "self")[0], cuda)
        for rc in (lib.df3d_bmap_prepare(Sd.data_ptr(), M, D, bo.FLOOR, pa[1], la[1], ea[1], va[1], st),
                   lib.df3d_bmap_prepare(Td.data_ptr(), N, D, bo.FLOOR, pb[1], lb[1], eb[1], vb[1], st),
                   lib.df3d_bmap_divergence(pa[1], ea[1], M, lb[1], N, D, Kt[1], st),
                   lib.df3d_bmap_calibrate(Kt[1], M, N, 10.0, bo.ENTROPY_TOL, bo.BETA_MAX, None, ct[1], bt[1], it[1], st),
                   lib.df3d_bmap_place(ct[1], M, N, Yd.data_ptr(), out[1], st),
                   lib.df3d_bmap_joint(cd.data_ptr(), N, Pj[1], st),
                   lib.df3d_bmap_cost(Pj[1], N, Yd.data_ptr(), cost[1], work[1], need, st)):
            assert rc == 0, lib.df3d_last_error()
        side.synchronize()
    got = {name: inner(t[0]) for name, t in dict(pa=pa, la=la, ea=ea, va=va, pb=pb, lb=lb, eb=eb, vb=vb, K=Kt, c=ct, b=bt, i=it, out=out, P=Pj,
                                                 cost=cost).items()}
    inner(work[0])
    for name, a in got.items():
        assert not np.any(a == (sentinel if a.dtype == np.float64 else -77)), f"{name} was not written everywhere"
    assert got["va"].all() and got["vb"].all() and not got["i"].any()
    p_a, p_b = bo.distributions(Sa)[0], bo.distributions(Sb)[0]
    assert np.all(np.abs(got["K"].reshape(M, N) - bo.divergence(p_a, p_b)) <= 2 * bo.divergence_tolerance(p_a, p_b))   # p itself is rounded twice here
    c = got["c"].reshape(M, N)
    bar = (N + 8) * bo.EPS * (np.abs(c) @ np.abs(want[0]))
    assert np.all(np.abs(got["out"].reshape(M, 2) - bo.place(c, want[0])) <= bar)
    assert np.array_equal(got["P"].reshape(N, N), bo.joint(cd.cpu().numpy()))
    assert abs(got["cost"][0] - bo.cost(bo.joint(cd.cpu().numpy()), want[0])) <= 1e-12


@pytest.mark.parametrize("N", [65, 257])
def test_free_running_trajectory(native_lib, cuda, N):
    """25 iterations from the same start.  The descent amplifies rounding, so the yardstick comes from the oracle itself: the
    largest deviation at iteration 25 among eight starts perturbed by a relative 1e-15.  The device rounds every N-term sum
    differently, not one entry once: it may differ from the unperturbed oracle by 16 times that."""
    from deepfly3d_amd import ops

    P, _ = bo.teacher_case(N)
    Y0 = bo.initial(N, N)
    ref = bo.run(P, Y0, 25)[0]
    yard = max(np.abs(bo.run(P, y, 25)[0] - ref).max() for y in bo.perturbed(Y0))
    got = ops.tsne(_dev(P, cuda), _dev(Y0, cuda), 25)[0].cpu().numpy()
    dev = np.abs(got - ref).max()
    print(f"N = {N}: the device is {dev:.3g} from the oracle after 25 iterations, the perturbed oracles up to {yard:.3g}: ratio {dev / yard:.3g} (bar 16)")
    assert yard > 0 and dev <= 16 * yard


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_planted_behaviours_end_to_end(native_lib, cuda):
    from deepfly3d_amd import ops

    full, lab, res, kls = bo.planted_case()
    c = bo.PLANTED
    r = ops.behaviour_map(_dev(full, cuda), c["perplexity"], c["n_iter"], c["max_points"], seed=0)
    emb = r.embedding.cpu().numpy()
    assert emb.shape == (184, 2) and emb.dtype == np.float64 and r.perplexity == 10.0 and isinstance(r.kl, float)
    assert np.array_equal(np.isnan(emb).any(axis=1), lab < 0) and np.array_equal(np.isnan(r.beta.cpu().numpy()), lab < 0)
    assert np.array_equal(r.train_index.cpu().numpy(), res["train_index"]) and r.train_index.dtype == torch.int64
    assert r.info.dtype == torch.int32 and not r.info.cpu().numpy().any()
    ok = lab >= 0
    assert np.abs(r.beta.cpu().numpy()[ok] / res["beta"][ok] - 1.0).max() <= 1e-6
    own_label, between, own = bo.separation(emb, lab)
    o_label, o_between, o_own = bo.separation(res["embedding"], lab)
    spread = float(np.ptp(kls))
    print(f"device: between-label {between:.3g}, own-label nearest neighbour up to {own:.3g}, KL {r.kl:.6f}; oracle: {o_between:.3g}, {o_own:.3g}, "
          f"KL {res['kl']:.6f}, its eight perturbed starts {kls.min():.6f} .. {kls.max():.6f} (spread {spread:.3g})")
    assert o_label and o_between >= 2 * o_own
    assert own_label and between >= 2 * own
    assert abs(r.kl - res["kl"]) <= 2 * spread
    # the same seed twice: the same bits
    again = ops.behaviour_map(_dev(full, cuda), c["perplexity"], c["n_iter"], c["max_points"], seed=0)
    assert again.embedding.cpu().numpy().tobytes() == emb.tobytes() and again.kl == r.kl


def test_shapes_through_ops(native_lib, cuda):
    from deepfly3d_amd import ops

    S, _ = bo.spectra(40, 6 * 8 * 3, seed=9)
    flat = ops.spectrogram_distributions(_dev(S, cuda))[0]
    p4, v4 = ops.spectrogram_distributions(_dev(S.reshape(40, 6, 8, 3), cuda))
    assert p4.shape == (40, 144) and torch.equal(p4, flat) and v4.shape == (40,)
    wide = _dev(np.repeat(S, 2, axis=1), cuda)[:, ::2]   # not contiguous: ops copies
    assert not wide.is_contiguous() and torch.equal(ops.spectrogram_distributions(wide)[0], flat)
    K = ops.kl_divergence(flat[::2], flat)   # a strided view of the rows
    assert K.shape == (20, 40) and torch.equal(K, ops.kl_divergence(flat[::2].contiguous(), flat))
    empty = torch.zeros((0, 6, 8, 3), dtype=torch.float64, device=cuda)
    p0, v0 = ops.spectrogram_distributions(empty)
    assert p0.shape == (0, 144) and v0.shape == (0,) and v0.dtype == torch.bool
    assert ops.kl_divergence(p0, flat).shape == (0, 40) and ops.kl_divergence(flat, p0).shape == (40, 0)
    c0 = ops.perplexity_calibrate(torch.zeros((0, 40), dtype=torch.float64, device=cuda), 4.0)
    assert c0[0].shape == (0, 40) and c0[1].shape == (0,) and c0[2].dtype == torch.int32
    P = ops.joint_probabilities(ops.perplexity_calibrate(ops.kl_divergence(flat, flat), 4.0, "self")[0])
    Y0 = _dev(bo.initial(40, 3), cuda)
    same = ops.tsne(P, Y0, 0)
    assert torch.equal(same[0], Y0) and not same[1].any() and torch.equal(same[2], torch.ones_like(Y0))   # no iterations: the start
    with pytest.raises(ValueError, match="at least one channel"):
        ops.spectrogram_distributions(torch.zeros((5, 0), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="S must be"):
        ops.spectrogram_distributions(torch.zeros((5, 2), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError, match="needs at least 97 frames"):
        ops.behaviour_map(empty)
    m = ops.behaviour_map(_dev(S.reshape(40, 6, 8, 3), cuda), perplexity=4, n_iter=20, max_points=16)
    assert m.embedding.shape == (40, 2) and m.train_index.shape == (16,) and torch.isfinite(m.embedding).all() and np.isfinite(m.kl)


# ------------------------------------------------------------------------------------------------------------------ Core and the CLI
def _recording(tmp_path, golden_dir):
    """(folder, result pickle): 15 frames (links to the sample's frame 0) and an earlier result holding the golden detections and cameras."""
    folder = tmp_path / "working"
    folder.mkdir()
    for c in range(7):
        for t in range(15):
            os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_{t}.jpg")
    folder = str(folder)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    os.makedirs(folder + "_df3d")
    pkl = os.path.join(folder + "_df3d", "df3d_result_" + os.path.abspath(folder).replace("/", "_") + ".pkl")
    res = {c: {"R": g3["R"][c], "tvec": g3["tvec"][c], "distort": g3["distort"][c], "intr": g3["intr"][c]} for c in range(7)}
    res.update(points2d=g3["points2d"], camera_ordering=g3["camera_ordering"], heatmap_confidence=g3["heatmap_confidence"])
    with open(pkl, "wb") as f:
        pickle.dump(res, f)
    return folder, pkl


def _load(pkl):
    with open(pkl, "rb") as f:
        return pickle.load(f)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


MAP_KEYS = ["behaviour_map", "behaviour_map_train_index", "behaviour_map_kl", "behaviour_map_perplexity"]


def _check_keys(run, rigid):
    T = 15
    for key in ["behaviour_map"] + (["behaviour_map_rigid"] if rigid else []):
        assert run[key].shape == (T, 2) and run[key].dtype == np.float64
    idx = run["behaviour_map_train_index"]
    assert idx.dtype == np.int64 and idx.ndim == 1 and 13 <= len(idx) <= T and np.all(np.diff(idx) > 0)
    finite = np.isfinite(run["behaviour_map"]).all(axis=1)
    assert finite[idx].all() and finite.sum() == len(idx)   # every valid frame trains: 15 <= max_points
    assert isinstance(run["behaviour_map_kl"], float) and np.isfinite(run["behaviour_map_kl"]) and run["behaviour_map_perplexity"] == 4.0
    if rigid:
        assert isinstance(run["behaviour_map_rigid_kl"], float) and np.isfinite(run["behaviour_map_rigid_kl"])


def test_core_behaviour_map(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    m = core.behaviour_map(perplexity=4)
    assert isinstance(m, ops.BehaviourMapResult) and all(isinstance(a, np.ndarray) for a in m[:4])
    assert m.embedding.shape == (15, 2) and m.beta.shape == (15,) and m.info.shape == (15,) and m.perplexity == 4.0
    # the map is the oracle's map of the float64 spectrogram: same training frames, same calibration
    S = core.angle_spectrogram()[0]
    p, valid = bo.distributions(S)
    assert np.array_equal(np.isfinite(m.embedding).all(axis=1), valid) and np.array_equal(m.train_index, np.flatnonzero(valid))
    want = bo.calibrate(bo.divergence(p[valid], p[valid]), 4.0, "self")
    assert np.abs(m.beta[valid] / want[1] - 1.0).max() <= 1e-6 and np.array_equal(m.info[valid], want[2])
    assert core.behaviour_map(perplexity=4, seed=0).embedding.tobytes() == m.embedding.tobytes()
    assert core.behaviour_map(perplexity=4, seed=1).embedding.tobytes() != m.embedding.tobytes()
    few = core.behaviour_map(perplexity=4, n_iter=10, num=8, f_max=20.0)   # the bank's arguments reach the spectrogram
    assert few.embedding.shape == (15, 2)
    with pytest.raises(ValueError, match="perplexity 32 needs at least 97 frames .* this recording has 15 valid frames"):
        core.behaviour_map()
    core.save(joint_angles=True, rigid_legs=True, angle_spectrogram=True)
    before = _load(pkl)
    core.save(joint_angles=True, rigid_legs=True, angle_spectrogram=True, behaviour_map=True, behaviour_perplexity=4)
    flagged = _load(pkl)
    assert list(flagged.keys()) == list(before.keys()) + MAP_KEYS + ["behaviour_map_rigid", "behaviour_map_rigid_kl"]
    assert all(_same(before[k], flagged[k]) for k in before)
    _check_keys(flagged, True)
    assert flagged["behaviour_map"].tobytes() == m.embedding.tobytes() and flagged["behaviour_map_kl"] == m.kl
    with pytest.raises(ValueError, match="needs at least 97 frames"):
        core.save(behaviour_map=True)
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_behaviour_map(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    folder, pkl = _recording(tmp_path, golden_dir)
    with open(pkl, "rb") as f:
        earlier = f.read()
    order = [str(c) for c in range(7)]

    def reopen(*flags):
        with open(pkl, "wb") as f:
            f.write(earlier)
        assert cli.main([folder, "--skip-pose-estimation", *flags, "--order"] + order) == 0
        return _load(pkl)

    keys = [str(k) for k in g3["key_order"]]
    rigid_keys = ["points3d_rigid", "rigid_segment_lengths", "rigid_fit_cost"]
    plain = reopen("--rigid-legs")
    run = reopen("--behaviour-map", "--behaviour-perplexity", "4", "--rigid-legs")
    assert [str(k) for k in run.keys()] == keys + rigid_keys + MAP_KEYS + ["behaviour_map_rigid", "behaviour_map_rigid_kl"]
    assert all(_same(plain[k], run[k]) for k in plain)   # every earlier key byte for byte; no angle_spectrogram key without its flag
    _check_keys(run, True)
    base = reopen("--joint-angles")
    only = reopen("--behaviour-map", "--behaviour-perplexity", "4", "--joint-angles")
    assert [str(k) for k in only.keys()] == keys + ["joint_angles", "segment_lengths"] + MAP_KEYS
    assert all(_same(base[k], only[k]) for k in base)
    _check_keys(only, False)
    assert _same(only["behaviour_map"], run["behaviour_map"])
    both = reopen("--behaviour-map", "--behaviour-perplexity", "4", "--angle-spectrogram")
    assert [str(k) for k in both.keys()] == keys + ["angle_spectrogram", "spectrogram_freqs", "spectrogram_fps"] + MAP_KEYS
    with open(pkl, "wb") as f:
        f.write(earlier)
    with pytest.raises(ValueError, match="perplexity 32 needs at least 97 frames .* this recording has 15 valid frames: the largest perplexity "
                                         r"accepted for 15 frames is 4\.667"):
        cli.main([folder, "--skip-pose-estimation", "--behaviour-map", "--order"] + order)
    with open(pkl, "rb") as f:
        assert f.read() == earlier   # refused before any work: the earlier result is untouched
    config.pop("image_shape", None)
