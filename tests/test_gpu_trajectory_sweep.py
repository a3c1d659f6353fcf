"""GPU sweep of the trajectory fit (csrc/trajectory.hip, DESIGN.md section 24, "swept"): the damped branch's rejected trials, chains that run
out of iterations or stall, a lambda per joint, chains of more than 256 blocks, 64 joints, 2 and 8 cameras, the solve's `ok`, and the
buffers' edges, on the families of tests/trajectory_cases.py against the float64 oracle tests/trajectory_oracle.py.

tests/test_trajectory_cases_host.py certifies the families: a chain named `firm` takes the same decisions along three host paths, and it
is compared exactly here -- status, counts, iterations, the start's cost bit for bit, the points within max(16 x the paths' largest
difference, STEP_TOL), errors and final cost within the bars derived in trajectory_cases.error_and_cost_bars.  A `structural` chain (a NaN
pivot, a NaN cost) ends at its start bit for bit.  Every other chain is held to invariants only.  Every comparison prints its figures
before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import trajectory_cases as tc
import trajectory_oracle as to
from deepfly3d_amd import config

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
FIELDS = ("points3d", "status", "weight", "error", "iterations", "cost", "counts")
SENTINEL, INT_SENTINEL = -12345.678, -77


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the families are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _fit(cuda, fam, B=None):
    """ops.triangulate_trajectory on a family, as numpy."""
    from deepfly3d_amd import ops

    r = ops.triangulate_trajectory(fam.P, _dev(fam.px, cuda), _dev(fam.X0, cuda), lam=fam.lam, huber=fam.huber, max_gap=fam.max_gap, block_frames=B)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in FIELDS}


def _base_status(fam, ref):
    nviews = to.views(fam.px).sum(axis=0)
    return np.where(ref["active"], np.where(ref["anchor"], 1, np.where(nviews >= 1, 2, 3)), 0).astype(np.int8)


def _invariants(fam, got, ref):
    """What holds of every chain, firm or not."""
    status, X, J = got["status"], got["points3d"], fam.px.shape[2]
    assert status.dtype == np.int8 and ((status >= 0) & (status <= 4)).all()
    assert np.array_equal(status != 0, ref["active"])
    base = _base_status(fam, ref)
    for j in range(J):
        ended = (status[:, j] == 4).any()
        assert np.array_equal(status[:, j], np.where(ref["active"][:, j], 4, 0) if ended else base[:, j]), j
    assert np.array_equal(got["counts"], np.stack([(status == k).sum(axis=0) for k in range(5)], axis=1))
    assert np.array_equal(_bits(X[status == 0]), _bits(fam.X0[status == 0]))          # an inactive frame keeps the input's bits
    assert not got["weight"][:, status == 0].any() and not got["error"][:, status == 0].any()
    cost, it = got["cost"], got["iterations"]
    assert (it >= 0).all() and (it <= config.TRAJECTORY_MAX_ITER).all()
    ok = ~np.isnan(cost[:, 0])
    assert (cost[ok, 1] <= cost[ok, 0] * (1.0 + config.TRAJECTORY_SLACK) ** it[ok]).all()
    assert np.array_equal(np.isnan(cost[:, 1]), ~ok)


def _firm(cuda, name, fam, got, ref, k, bar, B):
    """The chains k of a launch against the oracle's dict `ref` of the same launch."""
    k = list(k)
    sub, want = tc.chains_of(fam, k), tc.result_of(ref, k)
    error_bar, cost_bar = tc.error_and_cost_bars(sub.P, sub.px, want, sub.lam, sub.huber, bar)
    X, status, err, cost = got["points3d"][:, k], got["status"][:, k], got["error"][:, :, k], got["cost"][k]
    worst = float(np.abs(X - want["X"]).max()) if X.size else 0.0
    finite = np.isfinite(want["error"])
    worst_err = float((np.abs(err - want["error"])[finite] / error_bar[finite]).max()) if finite.any() else 0.0
    apart = np.abs(cost[:, 1] - want["cost"][:, 1])
    worst_cost = float(np.where(apart == 0.0, 0.0, apart / np.where(cost_bar > 0.0, cost_bar, 1.0)).max())
    print(f"{name} B {B}: {len(k)} firm chains, |device - oracle| {worst:.2e} mm (bar {bar:.2e}), errors at {worst_err:.2e} of their bar, final "
          f"cost at {worst_cost:.2e} of its bar, iterations {got['iterations'][k].tolist()[:8]} (oracle {want['iterations'].tolist()[:8]}), "
          f"ends {sorted(set(want['fit_status'].tolist()))}")
    assert np.array_equal(status, want["status"]) and np.array_equal(got["counts"][k], want["counts"])
    assert np.array_equal(got["iterations"][k], want["iterations"])
    assert np.array_equal(_bits(cost[:, 0]), _bits(want["cost"][:, 0]))                  # the start's cost: the oracle's operations, bit for bit
    assert worst <= bar
    assert np.array_equal(np.isfinite(err), finite) and np.array_equal(err == 0.0, want["error"] == 0.0)
    assert (np.abs(err - want["error"])[finite] <= error_bar[finite]).all()
    assert (np.abs(cost[:, 1] - want["cost"][:, 1]) <= cost_bar).all()
    # a view's weight is below 1 exactly where its error is above delta; compared where the oracle's error is not within its bar of delta
    clear = finite & (np.abs(want["error"] - sub.huber) > error_bar)
    assert np.array_equal((got["weight"][:, :, k] < 1.0)[clear], (want["weight"] < 1.0)[clear])
    for i, end in enumerate(want["fit_status"]):                                          # a chain that did not converge: status 4 throughout
        if end != to.CONVERGED:
            active = want["active"][:, i]
            assert (status[active, i] == 4).all() and got["counts"][k[i], 4] == active.sum() and not got["counts"][k[i], 1:4].any()


def _structural(cuda, fam, got, ref, k):
    """Chains that stall without an accepted trial: the start, bit for bit."""
    from deepfly3d_amd import ops

    start = to.start_points(fam.X0, ref["anchor"], ref["active"])
    _, _, weight, error, _ = (t.cpu().numpy() for t in ops.trajectory_linearize(fam.P, _dev(fam.px, cuda), _dev(start, cuda), huber=fam.huber))
    for j in k:
        active = ref["active"][:, j]
        assert active.any() and (got["status"][active, j] == 4).all() and got["counts"][j, 4] == active.sum() and got["iterations"][j] == 0
        assert np.array_equal(_bits(got["points3d"][:, j]), _bits(start[:, j]))
        assert np.array_equal(_bits(got["cost"][j, :1]), _bits(ref["cost"][j, :1])) and np.array_equal(_bits(got["cost"][j, 1:]), _bits(got["cost"][j, :1]))
        assert np.array_equal(_bits(got["weight"][:, :, j]), _bits(np.where(active[None], weight[:, :, j], 0.0)))
        assert np.array_equal(_bits(got["error"][:, :, j]), _bits(np.where(active[None], error[:, :, j], 0.0)))


def _against_oracle(cuda, name, blocks=tc.FIT_BLOCKS):
    fam, cert = tc.sweep(name), tc.certificate(name)
    bar, first = (tc.point_bar(name) if fam.firm else None), None
    for B in blocks:
        got = _fit(cuda, fam, B)
        _invariants(fam, got, cert.whole)
        if fam.structural:
            _structural(cuda, fam, got, cert.whole, fam.structural)
        if fam.firm:
            _firm(cuda, name, fam, got, cert.whole, fam.firm, bar, B)
            k = list(fam.firm)
            first = got["points3d"][:, k] if first is None else first
            assert float(np.abs(got["points3d"][:, k] - first).max()) <= bar            # two block sizes agree within the same bar
    return fam, cert


# ------------------------------------------------------------------------------------------------------------------ the damped branch
@pytest.mark.parametrize("name", ["rejected", "rejected_clean", "out_of_iterations", "per_joint_lambda", "mixed"])
def test_firm_chains_against_the_oracle(native_lib, cuda, name):
    """Rejected trials, 300 accepted ones, a lambda per chain, and every end in one launch; every chain here is firm or structural."""
    fam, cert = _against_oracle(cuda, name)
    assert len(fam.firm) + len(fam.structural) == fam.px.shape[2]
    if name in ("rejected", "rejected_clean", "mixed"):
        assert (cert.whole["iterations"][list(fam.firm)] < [len(s) for s in cert.three.strings["float64"]]).any()   # trials were rejected


@pytest.mark.parametrize("name", ["pivot_stall", "nan_cost_stall"])
def test_structural_stalls_end_at_their_start(native_lib, cuda, name):
    """Sixteen trials rejected at a NaN pivot (lambda = 1e308) or on a NaN cost (a start that overflows): status 4, no iteration, the
    start's points, cost, weights and errors bit for bit, at every block size."""
    fam, cert = _against_oracle(cuda, name)
    got = _fit(cuda, fam)
    print(f"{name}: cost {got['cost'].tolist()}, iterations {got['iterations'].tolist()}, counts {got['counts'].tolist()}")
    assert (cert.whole["fit_status"][list(fam.structural)] == to.STALLED).all()
    if name == "nan_cost_stall":
        assert np.isnan(got["cost"][0]).all() and np.isinf(got["points3d"][10, 0]).all() and got["counts"][1, 4] == 0


def test_chains_that_are_not_firm_keep_the_invariants(native_lib, cuda):
    """cost_stalled's chain 1 stalls on cost after about a hundred trials along sequences that differ between the host paths: no
    trajectory is compared.  Its status agrees with the oracle's active frames and with its own end, the cost never rises by more than
    the slack per accepted trial, inactive frames keep their bits and two runs give the same bits (_invariants); chain 0 is firm."""
    fam, cert = _against_oracle(cuda, "cost_stalled")
    assert fam.firm == (0,) and not fam.structural
    for B in tc.FIT_BLOCKS:
        a, b = _fit(cuda, fam, B), _fit(cuda, fam, B)
        print(f"cost_stalled B {B}: chain 1 ends with status {sorted(set(a['status'][:, 1].tolist()))} after {a['iterations'][1]} accepted trials "
              f"(oracle: {cert.whole['iterations'][1]}, stalled), cost {a['cost'][1].tolist()}")
        assert all(np.array_equal(_bits(a[f]), _bits(b[f])) for f in FIELDS)


# ------------------------------------------------------------------------------------------------------------------ shapes
def test_long_chains_whole_fit(native_lib, cuda):
    """T = 1025 at B = 3 (342 blocks: the lanes 0 .. 85 eliminate and substitute two), at the default block (33) and at the other block
    sizes, J = 2 and J = 1."""
    blocks = tc.FIT_BLOCKS + (config.trajectory_block_frames(1025),)
    fam, cert = _against_oracle(cuda, "long", blocks)
    assert set(np.unique(cert.whole["status"])) == {0, 1, 2, 3}
    one, bar = tc.chains_of(fam, [0]), tc.point_bar("long")
    ref = tc.result_of(cert.whole, [0])
    for B in blocks:
        got = _fit(cuda, one, B)
        _invariants(one, got, ref)
        _firm(cuda, "long, J = 1", one, got, ref, [0], bar, B)


@pytest.mark.parametrize("max_gap", [0, 1, 2, 5])
def test_segments_of_64_joints(native_lib, cuda, max_gap):
    """J = MAX_J = 64, every chain with its own anchor pattern, gaps either side of max_gap; the status also against the walk along a chain."""
    fam, cert = _against_oracle(cuda, f"segments{max_gap}")
    status = _fit(cuda, fam)["status"]
    walked = np.zeros(status.shape, bool)
    for j in range(64):
        for first, last in to.segments_loop(cert.whole["anchor"][:, j], max_gap):
            walked[first : last + 1, j] = True
    assert np.array_equal(status != 0, walked) and np.array_equal(status, _base_status(fam, cert.whole))


@pytest.mark.parametrize("ncam", [2, 8])
def test_two_and_eight_cameras(native_lib, cuda, ncam):
    fam, _ = _against_oracle(cuda, f"cameras{ncam}")
    assert fam.P.shape[0] == ncam


# ------------------------------------------------------------------------------------------------------------------ the solve
def _system(H, g, X, seg, lam):
    """(AB, b, G) of tc.solve_system for an H of the test's own and a lambda per chain."""
    active = seg != 0
    c = to.centres(active)
    G = g + lam[None, :, None] * to.smoothness(X, c)[1]
    AB, b = to.system(H, G, c, active, lam, np.full(len(lam), tc.SOLVE_MU))
    return AB, b, G


def _solve(cuda, H, G, seg, lam, B):
    from deepfly3d_amd import ops

    d, ok = ops.trajectory_solve(_dev(H, cuda), _dev(G, cuda), _dev(seg, cuda), lam, tc.SOLVE_MU, block_frames=B)
    d = d.cpu().numpy()
    return d, ok.cpu().numpy()


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_solve_reports_a_pivot_that_is_not_positive(native_lib, cuda, lam):
    """T = 40, J = 4: the H of one frame of chains 1 and 3 is -1e3 I, in a block's interior (chain 1) and on a separator frame (chain 3).
    A symmetric matrix with a negative diagonal entry is not positive definite, so some pivot is not positive in any order of
    elimination: ok = [1, 0, 1, 0], on the device and in the oracle.  Chains 0 and 2 are solved as if alone."""
    T, J = 40, 4
    H0, g, X = tc.solve_terms(T, J)
    lams = np.full(J, lam)
    for B in tc.SOLVE_BLOCKS:
        Bc = min(B, T)
        nb = -(-T // Bc)
        interior, separator = (Bc if nb > 1 else 5), Bc * (nb // 2) + Bc - 2
        seg = tc.segment_table(T, J, B)
        assert seg[interior, 1] and seg[separator, 3] and interior % Bc < Bc - 2 and separator % Bc == Bc - 2
        H = np.array(H0)
        H[interior, 1] = H[separator, 3] = (-1e3, 0.0, 0.0, -1e3, 0.0, -1e3)
        AB, b, G = _system(H, g, X, seg, lams)
        d, ok = _solve(cuda, H, G, seg, lams, B)
        ref, ref_ok = to.banded_solve(AB, b)
        x = d.transpose(1, 0, 2).reshape(J, 3 * T)
        good = [0, 2]
        mine, theirs = to.backward_error(AB[good], b[good], x[good]), to.backward_error(AB[good], b[good], ref[good])
        print(f"lambda {lam:g} B {B}: ok {ok.tolist()} (oracle {ref_ok.astype(int).tolist()}), chains 0 and 2: device {mine.max():.2e} oracle {theirs.max():.2e}")
        assert ok.tolist() == [1, 0, 1, 0] and ref_ok.tolist() == [True, False, True, False]
        assert (mine <= 8.0 * np.maximum(theirs, EPS)).all()
        assert not d[:, good][seg[:, good] == 0].any()


def test_solve_takes_each_chains_own_lambda(native_lib, cuda):
    """lambda = (0, 1, 1e4, 1e8) in one call: each chain has the bits of the same chain solved alone with its own lambda."""
    T, J = 40, 4
    H, g, X = tc.solve_terms(T, J)
    lams = np.array(tc.SOLVE_LAMBDAS)
    for B in tc.SOLVE_BLOCKS:
        seg = tc.segment_table(T, J, B)
        G = _system(H, g, X, seg, lams)[2]
        d, ok = _solve(cuda, H, G, seg, lams, B)
        assert ok.all()
        for j in range(J):
            alone, ok1 = _solve(cuda, H[:, j : j + 1], G[:, j : j + 1], seg[:, j : j + 1], lams[j : j + 1], B)
            assert ok1.all() and np.array_equal(_bits(alone[:, 0]), _bits(d[:, j])), (B, j)
        assert not np.array_equal(d[:, 1], _solve(cuda, H, G, seg, np.full(J, lams[0]), B)[0][:, 1])   # and lambda matters


@pytest.mark.parametrize("lam", [0.0, 1e4])
def test_solve_of_more_than_256_blocks(native_lib, cuda, lam):
    """B = 3 at T = 769 (257 blocks: lane 0 alone takes a second), 771 and 1025 (342), against the backward-error bar of the solve test:
    8 x max(the oracle's own banded factorisation on the same system, eps)."""
    J = 3
    for T in (769, 771, 1025):
        AB, b, seg, G = tc.solve_system(T, J, 3, lam)
        d, ok = _solve(cuda, tc.solve_terms(T, J)[0], G, seg, np.full(J, lam), 3)
        assert ok.all() and not d[seg == 0].any()
        x = d.transpose(1, 0, 2).reshape(J, 3 * T)
        ref, ref_ok = to.banded_solve(AB, b)
        mine, theirs = to.backward_error(AB, b, x), to.backward_error(AB, b, ref)
        print(f"lambda {lam:g} T {T} B 3 ({-(-T // 3)} blocks): device {mine.max():.2e} oracle {theirs.max():.2e}")
        assert ref_ok.all() and (mine <= 8.0 * np.maximum(theirs, EPS)).all(), (T, float(mine.max()), float(theirs.max()))


# ------------------------------------------------------------------------------------------------------------------ bit for bit
def test_a_chain_is_the_same_bits_alone_or_in_company(native_lib, cuda):
    """Each chain of `mixed` in a J = 1 call with its own lambda against the J = 5 launch, whose workgroups leave the loop after 0, 16,
    82, 90 and 300 trials; the launch twice, and once more on a side stream."""
    fam = tc.sweep("mixed")
    for B in (3, 16):
        whole = _fit(cuda, fam, B)
        assert sorted(whole["iterations"].tolist()) == [0, 0, 37, 90, 300]
        for j in range(fam.px.shape[2]):
            alone = _fit(cuda, tc.chains_of(fam, [j]), B)
            for f in FIELDS:
                mine = whole[f][:, :, j : j + 1] if f in ("weight", "error") else whole[f][:, j : j + 1] if f in ("points3d", "status") else whole[f][j : j + 1]
                assert np.array_equal(_bits(alone[f]), _bits(mine)), (B, j, f)
        again = _fit(cuda, fam, B)
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            aside = _fit(cuda, fam, B)
        for f in FIELDS:
            assert np.array_equal(_bits(again[f]), _bits(whole[f])) and np.array_equal(_bits(aside[f]), _bits(whole[f])), (B, f)


# ------------------------------------------------------------------------------------------------------------------ guard words
GUARD = 1 << 20          # bytes either side of every buffer


class _Guarded:
    """`count` elements of `dtype` in the middle of a sentinel-filled allocation."""

    def __init__(self, cuda, count, dtype):
        self.n, self.g = count, GUARD // torch.empty((), dtype=dtype).element_size()
        self.fill = SENTINEL if dtype == torch.float64 else 0xA5 if dtype == torch.uint8 else INT_SENTINEL
        self.whole = torch.full((self.g + count + self.g,), self.fill, dtype=dtype, device=cuda)
        self.part = self.whole[self.g : self.g + count]
        self.ptr = self.part.data_ptr()

    def guards_untouched(self):
        return bool((self.whole[: self.g] == self.fill).all()) and bool((self.whole[self.g + self.n :] == self.fill).all())

    def all_written(self):
        return not bool((self.part == self.fill).any())


@pytest.mark.parametrize("T,B,J", [(5, 3, 1), (40, 16, 38), (40, 1 << 20, 2), (257, 7, 3)])
def test_guard_words_around_every_buffer(native_lib, cuda, T, B, J):
    """df3d_triangulate_trajectory and df3d_trajectory_solve through the C ABI with work_bytes exactly as df3d_trajectory_work_bytes gives
    it (the solve also with its own part of it, J (48 nb Bc + 105 nb) doubles); the padded chain nb Bc is longer than T in all four
    shapes.  Every output and the work buffer are slices of sentinel-filled allocations: the guards stay, every output element is written."""
    lib, dp = native_lib, ctypes.POINTER(ctypes.c_double)
    P, px = tc.fly(T)[:2] if J == 38 else tc.outliers(3, T, J)[:2]
    ncam, Bc = P.shape[0], min(B, max(T, 3))
    nb = -(-T // Bc)
    assert nb * Bc > T or B == 1 << 20               # (one block of exactly T frames there)
    lam = np.ascontiguousarray(np.linspace(1e2, 1e4, J))
    Ph = np.ascontiguousarray(P, dtype=np.float64)
    need = lib.df3d_trajectory_work_bytes(ncam, T, J, B)
    assert need > 0 and need % 8 == 0
    pts, X0 = _dev(px, cuda), _dev(tc.dlt(P, px), cuda)
    out = dict(X=_Guarded(cuda, T * J * 3, torch.float64), status=_Guarded(cuda, T * J, torch.int8), weight=_Guarded(cuda, ncam * T * J, torch.float64),
               error=_Guarded(cuda, ncam * T * J, torch.float64), iterations=_Guarded(cuda, J, torch.int32), cost=_Guarded(cuda, J * 2, torch.float64),
               counts=_Guarded(cuda, J * 5, torch.int64))
    work = _Guarded(cuda, need, torch.uint8)
    rc = lib.df3d_triangulate_trajectory(Ph.ctypes.data_as(dp), pts.data_ptr(), X0.data_ptr(), ncam, T, J, lam.ctypes.data_as(dp), tc.HUBER, 10, B,
                                         out["X"].ptr, out["status"].ptr, out["weight"].ptr, out["error"].ptr, out["iterations"].ptr, out["cost"].ptr,
                                         out["counts"].ptr, work.ptr, need, None)
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()
    touched = [k for k, v in out.items() if not v.guards_untouched()] + ([] if work.guards_untouched() else ["work"])
    unwritten = [k for k, v in out.items() if not v.all_written()]
    print(f"fit T {T} B {B} J {J}: work {need} bytes, guards touched {touched}, outputs not wholly written {unwritten}")
    assert not touched and not unwritten
    ref = to.fit(P, px, X0.cpu().numpy(), lam, tc.HUBER, 10)
    assert np.array_equal(out["status"].part.view(T, J).cpu().numpy(), ref["status"])
    # the solve
    H, g, X = tc.solve_terms(T, J)
    seg = tc.segment_table(T, J, B)
    G = _system(H, g, X, seg, lam)[2]
    own = J * (48 * nb * Bc + 105 * nb) * 8
    assert own <= lib.df3d_trajectory_work_bytes(1, T, J, B)
    for size in (lib.df3d_trajectory_work_bytes(1, T, J, B), own):
        d, ok, work = _Guarded(cuda, T * J * 3, torch.float64), _Guarded(cuda, J, torch.int32), _Guarded(cuda, size, torch.uint8)
        Hd, Gd, sd = _dev(H, cuda), _dev(G, cuda), _dev(seg, cuda)
        rc = lib.df3d_trajectory_solve(Hd.data_ptr(), Gd.data_ptr(), sd.data_ptr(), T, J, lam.ctypes.data_as(dp), tc.SOLVE_MU, B, d.ptr, ok.ptr, None,
                                       work.ptr, size, None)
        assert rc == 0, lib.df3d_last_error()
        torch.cuda.synchronize()
        print(f"solve T {T} B {B} J {J}: work {size} bytes, guards untouched {d.guards_untouched(), ok.guards_untouched(), work.guards_untouched()}")
        assert d.guards_untouched() and ok.guards_untouched() and work.guards_untouched() and d.all_written() and ok.all_written()
        assert ok.part.cpu().numpy().all()
