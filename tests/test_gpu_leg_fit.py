"""GPU tests of the constant-length leg fit: ops.fit_legs / df3d_leg_fit against the float64 oracle
tests/leg_fit_oracle.py after one and two iterations and converged, on the golden recording and on synthetic flies, over the sizes
that cross a wave, a block and a partial last block with every way of choosing lengths and anchor; in place, inside guard words, on
poses with defects, against the closed-form replay, under rigid motions and scales; ops.segment_length_medians;
Core.joint_angles(rigid=True), Core.rigid_legs, Core.save and --rigid-legs end to end.

Bars (leg_fit_oracle.STEP_BAR, CONVERGED_BAR, COST_RTOL; section 15 has the measurements they are ten times of).  Every comparison
prints its figure before it asserts; no leg is excluded anywhere."""
import os
import pickle

import numpy as np
import pytest
import torch

import leg_fit_oracle as lo

pytestmark = pytest.mark.gpu

LENGTH_RTOL = 1e-12
RIGID_COST = 1e-24   # mm^2: below it a cost is that of an exact fit (tests/test_leg_fit_host.py), and relative differences mean nothing
LEGS = [j for leg in range(6) for j in lo.leg_joints(leg)]
OTHERS = [j for j in range(38) if j not in LEGS]


def _dev(cuda, a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(cuda)   # a copy: the shared fixtures are read-only


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _compare(fit, want, what, bar, iters_slack=0):
    """fit: a LegFitResult; want: the oracle's (points, cost, status, iters)."""
    pts, cost, status, iters = (_host(a) for a in (fit.points, fit.cost, fit.status, fit.iters))
    wp, wc, ws, wi = want
    assert pts.shape == wp.shape and cost.shape == wc.shape and status.dtype == np.int32 and iters.dtype == np.int32
    both = np.isfinite(wp)   # a leg that is not fitted may hold NaN or infinity: the input's bits, on both sides
    assert pts[~both].tobytes() == wp[~both].tobytes() and np.array_equal(np.isnan(cost), np.isnan(wc)), what
    dp = float(np.abs(pts[both] - wp[both]).max()) if both.any() else 0.0
    keep = wc > RIGID_COST   # NaN compares false; a leg that fits exactly has a cost of rounding errors only, on both sides
    dc = float((np.abs(cost[keep] - wc[keep]) / wc[keep]).max()) if keep.any() else 0.0
    assert (cost[wc <= RIGID_COST] <= RIGID_COST).all(), what
    di = int(np.abs(iters - wi).max()) if iters.size else 0
    print(f"{what}: points off by {dp:.3e} mm, cost by {dc:.3e} relative, iterations by {di}")
    assert np.array_equal(status, ws), what
    assert dp <= bar and dc <= lo.COST_RTOL and di <= iters_slack, what
    return dp, dc


_memo = {}


def _oracle(X, L, anchor=None, max_iter=lo.MAX_ITER):
    """lo.fit_legs with every leg's fit remembered by its inputs' bits: the sizes share frames, and a leg's fit depends on nothing but
    its own five joints, four lengths and anchor."""
    X = np.asarray(X, dtype=np.float64)
    out = X.copy()
    T = len(X)
    E, status, iters = np.full((T, 6), np.nan), np.zeros((T, 6), dtype=np.int32), np.zeros((T, 6), dtype=np.int32)
    for t in range(T):
        for leg in range(6):
            j = lo.leg_joints(leg)
            a = None if anchor is None else np.asarray(anchor, dtype=np.float64)[leg]
            key = (X[t, j].tobytes(), np.asarray(L, dtype=np.float64)[leg].tobytes(), None if a is None else a.tobytes(), max_iter)
            if key not in _memo:
                _memo[key] = lo.fit_leg(X[t, j], L[leg], a, max_iter)
            out[t, j], E[t, leg], status[t, leg], iters[t, leg] = _memo[key]
    return out, E, status, iters


@pytest.fixture(scope="module")
def sets(golden_dir):
    """{name: (X, lengths, anchor)}: the golden recording with its median lengths, anchored per frame; 40 seeded synthetic flies with the
    same lengths, noise of 0.02 x the mean length and an offset anchor."""
    X = np.load(f"{golden_dir}/golden_3d.npz")["points3d_wo_procrustes"]
    L = lo.median_lengths(X)
    Xs, A, _ = lo.synthetic_flies(np.random.default_rng(15), 40, L)
    for a in (X, L, Xs, A):
        a.setflags(write=False)
    return {"golden": (X, L, None), "synthetic": (Xs, L, A)}


@pytest.fixture(scope="module")
def tiled(sets):
    """[257, 38, 3]: 61 golden frames with seeded jitter of 5 um on every joint, repeated with period 61, so that no frame equals the
    frame 64 before it and the oracle fits 61 poses for every size."""
    X = sets["golden"][0]
    rng = np.random.default_rng(61)
    base = X[np.arange(61) % len(X)] + rng.normal(0.0, 0.005, (61, 38, 3))
    Z = np.ascontiguousarray(base[np.arange(257) % 61])
    Z.setflags(write=False)
    return Z


# ------------------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("max_iter", [1, 2])
@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_one_and_two_iterations_differ_by_rounding_only(native_lib, cuda, sets, name, max_iter):
    from deepfly3d_amd import ops

    X, L, A = sets[name]
    fit = ops.fit_legs(_dev(cuda, X), L, "per_frame" if A is None else A, max_iter=max_iter)
    want = _oracle(X, L, A, max_iter)
    assert (want[3] == max_iter).all() and (want[2] == lo.OUT_OF_ITERATIONS).all()   # nobody converges in two steps: same steps on both sides
    _compare(fit, want, f"{name}, max_iter = {max_iter}", lo.STEP_BAR)


@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_converged_fit_matches_the_oracle(native_lib, cuda, sets, name):
    from deepfly3d_amd import ops

    X, L, A = sets[name]
    fit = ops.fit_legs(_dev(cuda, X), L, "per_frame" if A is None else A)
    assert fit.points.device == cuda and tuple(fit.points.shape) == X.shape and tuple(fit.cost.shape) == (len(X), 6)
    assert tuple(fit.status.shape) == (len(X), 6) == tuple(fit.iters.shape) and np.array_equal(fit.lengths, L)
    want = _oracle(X, L, A)
    variant = lo.fit_legs(X, L, A, basis_variant=True)
    print(f"{name}: the oracle's own sensitivity to the tangent basis {np.abs(variant[0] - want[0]).max():.3e} mm")
    _compare(fit, want, f"{name}, converged", lo.CONVERGED_BAR, iters_slack=1)
    status, iters = _host(fit.status), _host(fit.iters)
    assert (status == lo.CONVERGED).all() and iters.max() <= 6
    got = lo.segment_lengths(_host(fit.points))
    assert np.abs(got / L - 1.0).max() <= LENGTH_RTOL
    assert np.array_equal(_host(fit.points)[:, OTHERS], X[:, OTHERS])


@pytest.mark.parametrize("anchor", ["per_frame", "recording", "explicit"])
@pytest.mark.parametrize("lengths", ["recording", "explicit"])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_sizes_across_wave_and_block_boundaries(native_lib, cuda, sets, tiled, T, lengths, anchor):
    from deepfly3d_amd import ops

    Z = tiled[:T]
    rng = np.random.default_rng(7)
    L = lo.median_lengths(Z) if lengths == "recording" else sets["golden"][1] * rng.uniform(0.97, 1.03, (6, 4))
    A = {"per_frame": None, "recording": lo.recording_anchor(Z), "explicit": lo.recording_anchor(tiled) + rng.normal(0.0, 0.01, (6, 3))}[anchor]
    fit = ops.fit_legs(_dev(cuda, Z), "recording" if lengths == "recording" else L, anchor if anchor != "explicit" else A)
    if lengths == "recording":   # the medians are exact on both sides; the lengths under them differ by rounding
        assert np.abs(fit.lengths / L - 1.0).max() <= LENGTH_RTOL
        L = fit.lengths
    want = _oracle(Z, L, A)
    _compare(fit, want, f"T = {T}, lengths {lengths}, anchor {anchor}", lo.CONVERGED_BAR, iters_slack=1)
    assert np.array_equal(_host(fit.points)[:, OTHERS], Z[:, OTHERS])
    if anchor == "recording":
        assert np.array_equal(_host(fit.points)[:, lo.COXAE], np.broadcast_to(A, (T, 6, 3)))


def test_max_iter_zero_is_the_replay(native_lib, cuda, sets):
    from deepfly3d_amd import ops

    for name, (X, L, A) in sets.items():
        fit = ops.fit_legs(_dev(cuda, X), L, "per_frame" if A is None else A, max_iter=0)
        want = X.copy()
        for t in range(len(X)):
            for leg in range(6):
                j = lo.leg_joints(leg)
                want[t, j] = lo.replay(X[t, j], L[leg], None if A is None else A[leg])
        diff = np.abs(_host(fit.points) - want).max()
        print(f"{name}: max_iter = 0 against the closed-form replay {diff:.3e} mm")
        assert diff <= lo.STEP_BAR and (_host(fit.status) == lo.OUT_OF_ITERATIONS).all() and (_host(fit.iters) == 0).all()
        _compare(fit, _oracle(X, L, A, 0), f"{name}, max_iter = 0", lo.STEP_BAR)


# ------------------------------------------------------------------------------------------------------------------ buffers
def _call(lib, X, L, A, out, cost, info, max_iter=lo.MAX_ITER):
    import ctypes

    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    L = np.ascontiguousarray(L, dtype=np.float64)
    A = None if A is None else np.ascontiguousarray(A, dtype=np.float64)
    rc = lib.df3d_leg_fit(X.data_ptr(), X.shape[0], ptr(L), None if A is None else ptr(A), max_iter, out.data_ptr(), cost.data_ptr(), info.data_ptr(), None)
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()


def test_in_place_guard_words_and_untouched_joints(native_lib, cuda, sets, tiled):
    from deepfly3d_amd import ops

    sentinel, guard = -12345.678, 16
    L = sets["golden"][1]
    for T, A in ((1, None), (65, None), (200, lo.recording_anchor(tiled))):
        Z = tiled[:T]
        ref = ops.fit_legs(_dev(cuda, Z), L, "per_frame" if A is None else A)
        n = T * 114
        # out of place into sentinel-filled buffers with guard words on both sides: the 30 leg joints are written, nothing else is
        out = torch.full((guard + n + guard,), sentinel, dtype=torch.float64, device=cuda)
        cost = torch.full((guard + T * 6 + guard,), sentinel, dtype=torch.float64, device=cuda)
        info = torch.full((guard + T * 12 + guard,), -77, dtype=torch.int32, device=cuda)
        _call(native_lib, _dev(cuda, Z), L, A, out[guard:guard + n], cost[guard:guard + T * 6], info[guard:guard + T * 12])
        assert (out[:guard] == sentinel).all() and (out[guard + n:] == sentinel).all()
        assert (cost[:guard] == sentinel).all() and (cost[guard + T * 6:] == sentinel).all()
        assert (info[:guard] == -77).all() and (info[guard + T * 12:] == -77).all()
        pts = out[guard:guard + n].view(T, 38, 3)
        assert (pts[:, OTHERS] == sentinel).all() and not (pts[:, LEGS] == sentinel).any()   # the caller fills the other joints
        assert torch.equal(pts[:, LEGS], ref.points[:, LEGS]) and torch.equal(cost[guard:guard + T * 6].view(T, 6), ref.cost)
        words = info[guard:guard + T * 12].view(T, 6, 2)
        assert torch.equal(words[..., 0], ref.status) and torch.equal(words[..., 1], ref.iters)
        # in place: bit-equal to out of place, the other joints untouched
        Zd = _dev(cuda, Z)
        _call(native_lib, Zd, L, A, Zd, cost[guard:guard + T * 6], info[guard:guard + T * 12])
        assert torch.equal(Zd, ref.points) and torch.equal(cost[guard:guard + T * 6].view(T, 6), ref.cost)
        assert np.array_equal(_host(Zd)[:, OTHERS], Z[:, OTHERS])


# ------------------------------------------------------------------------------------------------------------------ legs that are not fitted
def test_legs_that_are_not_fitted(native_lib, cuda, sets):
    from deepfly3d_amd import ops

    X, L, _ = sets["golden"]
    A = lo.recording_anchor(X)
    values = [("zeros", [0.0, 0.0, 0.0]), ("NaN", [1.0, np.nan, 2.0]), ("inf", [-np.inf, 3.0, 1.0])]
    poses, where = [X[2]], []
    for k in range(5):
        for n, (tag, value) in enumerate(values):
            leg = (k + 2 * n) % 6
            Y = X[2].copy()
            Y[lo.leg_joints(leg)[k]] = value
            poses.append(Y)
            where.append((k, tag, leg))
    for leg, k in ((0, 2), (4, 4)):   # coincident joints
        Y = X[2].copy()
        Y[lo.leg_joints(leg)[k]] = Y[lo.leg_joints(leg)[k - 1]]
        poses.append(Y)
        where.append((k, "coincident", leg))
    Y = np.stack(poses)
    for anchor in (None, A):
        fit = ops.fit_legs(_dev(cuda, Y), L, "per_frame" if anchor is None else anchor)
        _compare(fit, _oracle(Y, L, anchor), f"defects, anchor {'given' if anchor is not None else 'per frame'}", lo.CONVERGED_BAR, iters_slack=1)
        pts, cost, status, iters = (_host(a) for a in (fit.points, fit.cost, fit.status, fit.iters))
        assert (status[0] == lo.CONVERGED).all()
        for i, (k, tag, leg) in enumerate(where, start=1):
            others = [x for x in range(6) if x != leg]
            rest = [j for x in others for j in lo.leg_joints(x)]
            assert pts[i, rest].tobytes() == pts[0, rest].tobytes() and np.array_equal(cost[i, others], cost[0, others]), (k, tag)   # untouched legs
            assert np.array_equal(status[i, others], status[0, others]) and np.array_equal(iters[i, others], iters[0, others])
            j = lo.leg_joints(leg)
            if k == 0 and anchor is not None and tag != "coincident":   # the anchor stands in for the missing body-coxa joint
                assert status[i, leg] == lo.CONVERGED and pts[i, j].tobytes() == pts[0, j].tobytes(), tag
            else:
                assert status[i, leg] == lo.NOT_FITTED and iters[i, leg] == -1 and np.isnan(cost[i, leg]), (k, tag)
                assert pts[i, j].tobytes() == Y[i, j].tobytes(), (k, tag)   # the input's bits
        assert pts[:, OTHERS].tobytes() == Y[:, OTHERS].tobytes()


# ------------------------------------------------------------------------------------------------------------------ equivariance
def test_rigid_motion_and_scale(native_lib, cuda, sets):
    from deepfly3d_amd import ops

    X, L, _ = sets["golden"]
    A = lo.recording_anchor(X) + 0.01
    rng = np.random.default_rng(5)
    centre = X[:, LEGS].mean(axis=(0, 1))
    for anchor in (None, A):
        base = _host(ops.fit_legs(_dev(cuda, X), L, "per_frame" if anchor is None else anchor).points)
        R = lo.random_rotation(rng)
        shift = rng.normal(0.0, 0.2, 3)
        move = lambda P: (P - centre) @ R.T + centre + shift   # noqa: E731  (about the legs' centre: coordinates keep their size)
        got = _host(ops.fit_legs(_dev(cuda, move(X)), L, "per_frame" if anchor is None else move(anchor)).points)
        diff = np.abs(got - move(base))[:, LEGS].max()
        print(f"rigid motion, anchor {'given' if anchor is not None else 'per frame'}: {diff:.3e} mm")
        assert diff <= lo.CONVERGED_BAR
        for scale in (0.013, 250.0):
            got = _host(ops.fit_legs(_dev(cuda, scale * X), scale * L, "per_frame" if anchor is None else scale * anchor).points)
            diff = np.abs(got - scale * base)[:, LEGS].max()
            print(f"scale {scale}, anchor {'given' if anchor is not None else 'per frame'}: {diff:.3e} mm = {diff / scale:.3e} x the scale")
            assert diff <= lo.CONVERGED_BAR * scale


# ------------------------------------------------------------------------------------------------------------------ the median lengths
def test_segment_length_medians(native_lib, cuda, sets, tiled):
    from deepfly3d_amd import ops

    for X in (sets["golden"][0], tiled[:64]):
        Xd = _dev(cuda, X)
        M = ops.segment_length_medians(Xd)
        assert M.device == cuda and tuple(M.shape) == (6, 4)
        assert np.array_equal(_host(M), np.median(_host(ops.joint_angles(Xd, "per_frame")[1]), axis=0))   # exact medians of the device's lengths
        assert np.abs(_host(M) / lo.median_lengths(X) - 1.0).max() <= LENGTH_RTOL
    Y = sets["golden"][0].copy()
    Y[0, 7] = 0.0                    # leg 1's femur-tibia joint: its femur and tibia do not count in frames 0 and 1
    Y[1, 7, 2] = np.nan
    Y[:14, lo.leg_joints(5)[4]] = 0.0   # one frame left for leg 5's tarsus
    Yd = _dev(cuda, Y)
    with np.errstate(all="ignore"):
        want = np.nanmedian(_host(ops.joint_angles(Yd, "per_frame")[1]), axis=0)
    assert not np.isnan(want).any() and np.array_equal(_host(ops.segment_length_medians(Yd)), want)
    Y[14, lo.leg_joints(5)[4]] = np.inf
    with pytest.raises(ValueError, match=r"leg 5 \(side1_hind\), segment 3 \(tarsus\)"):
        ops.segment_length_medians(_dev(cuda, Y))
    with pytest.raises(ValueError, match="leg 5"):
        ops.fit_legs(_dev(cuda, Y))
    fit = ops.fit_legs(_dev(cuda, Y[:0]), sets["golden"][1])   # no poses, explicit lengths: nothing is launched
    assert tuple(fit.points.shape) == (0, 38, 3) and tuple(fit.cost.shape) == (0, 6) and tuple(fit.status.shape) == (0, 6)


# ------------------------------------------------------------------------------------------------------------------ strided poses
def test_a_strided_pose_gives_what_its_contiguous_copy_gives(native_lib, cuda, tiled):
    """Every wrapper that takes a pose [T, 38, 3] accepts any strides and works on the contiguous tensor: V = X[::2] gives the bytes
    of V.contiguous(), output by output (the outputs hold NaN), and V is not changed.  A wrapper that checked V and then handed
    V.data_ptr() and T = 5 to its kernel would read X[0:5], which the jitter of `tiled` makes another recording."""
    from deepfly3d_amd import ops

    X = tiled[:10].copy()
    X[4, lo.leg_joints(2)[3]] = 0.0      # a missing joint in a frame the view keeps
    X[3, lo.leg_joints(4)[1]] = np.nan   # and one in a frame it skips
    V = _dev(cuda, X)[::2]
    C = V.contiguous()
    assert tuple(V.shape) == (5, 38, 3) and not V.is_contiguous() and not np.array_equal(X[::2][1:], X[1:5], equal_nan=True)
    before = V.cpu().numpy().tobytes()

    def fit(points3d):
        r = ops.fit_legs(points3d, max_iter=2)
        return r.points, r.cost, r.status, r.iters

    calls = {"body_frame": ops.body_frame, "joint_angles per_frame": lambda p: ops.joint_angles(p, "per_frame"),
             "joint_angles recording": lambda p: ops.joint_angles(p, "recording"), "segment_length_medians": ops.segment_length_medians,
             "fit_legs": fit, "tip_kinematics": lambda p: ops.tip_kinematics(p, fps=100.0), "pose_outliers": ops.pose_outliers}
    for name, call in calls.items():
        got, want = call(V), call(C)
        got, want = ((got,), (want,)) if isinstance(got, torch.Tensor) else (got, want)
        assert len(got) == len(want) and len(got) >= 1, name
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.dtype == w.dtype and g.shape[0] in (5, 6), (name, i)
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (name, i)
        assert V.cpu().numpy().tobytes() == before and not V.is_contiguous(), name


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
    """Byte-identical values of a result (arrays, or the cameras' dictionaries of arrays)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


RIGID_KEYS = ["points3d_rigid", "rigid_segment_lengths", "rigid_fit_cost"]


def test_core_and_cli_end_to_end(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli, ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    folder, pkl = _recording(tmp_path, golden_dir)
    with open(pkl, "rb") as f:
        earlier = f.read()
    order = [str(c) for c in range(7)]
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    assert core.has_calibration and core.camNet.points3d is None
    pts, lengths, cost = core.rigid_legs()   # triangulates first
    assert all(isinstance(a, np.ndarray) for a in (pts, lengths, cost)) and pts.shape == (15, 38, 3) and lengths.shape == (6, 4) and cost.shape == (15, 6)
    X = core.camNet.points3d
    fit = ops.fit_legs(_dev(cuda, X))
    assert np.array_equal(pts, _host(fit.points)) and np.array_equal(lengths, fit.lengths) and np.array_equal(cost, _host(fit.cost))
    _compare(fit, _oracle(X, fit.lengths), "Core.rigid_legs", lo.CONVERGED_BAR, iters_slack=1)
    # joint_angles(rigid=True): the fixed lengths, the angles of the fitted pose in the measured pose's recording frame
    for mode in ("recording", "per_frame"):
        angles, seg = core.joint_angles(mode, rigid=True)
        assert np.abs(seg / lengths - 1.0).max() <= LENGTH_RTOL
        want = ops.joint_angles(fit.points, mode)   # anchored per frame, the body-coxa joints and so the frames are the measured pose's
        assert np.array_equal(angles, _host(want[0])) and np.array_equal(seg, _host(want[1]))
        assert not np.array_equal(angles, core.joint_angles(mode)[0])
    A = lo.recording_anchor(X) + 0.02
    moved = core.rigid_legs(lengths=lengths * 1.01, anchor=A)
    assert np.array_equal(moved[1], lengths * 1.01) and np.array_equal(moved[0][:, lo.COXAE], np.broadcast_to(A, (15, 6, 3)))
    # save: the keys after every existing one
    core.save(joint_angles=True)
    before = _load(pkl)
    core.save(joint_angles=True, rigid_legs=True)
    flagged = _load(pkl)
    assert list(flagged.keys()) == list(before.keys()) + RIGID_KEYS + ["joint_angles_rigid"]
    assert all(_same(before[k], flagged[k]) for k in before)
    assert np.array_equal(flagged["points3d_rigid"], pts) and np.array_equal(flagged["rigid_segment_lengths"], lengths)
    assert np.array_equal(flagged["rigid_fit_cost"], cost) and np.array_equal(flagged["joint_angles_rigid"], core.joint_angles(rigid=True)[0])
    core.save(rigid_legs=True)
    assert list(_load(pkl).keys()) == [k for k in before.keys() if k not in ("joint_angles", "segment_lengths")] + RIGID_KEYS
    # df3d-cli --skip-pose-estimation on the same earlier result, without and with the flags: every earlier key byte-identical
    def reopen(*flags):
        with open(pkl, "wb") as f:
            f.write(earlier)
        assert cli.main([folder, "--skip-pose-estimation", *flags, "--order"] + order) == 0
        return _load(pkl)

    plain = reopen("--joint-angles")
    assert [str(k) for k in plain.keys()] == [str(k) for k in g3["key_order"]] + ["joint_angles", "segment_lengths"]
    run = reopen("--rigid-legs", "--joint-angles")
    assert list(run.keys()) == list(plain.keys()) + RIGID_KEYS + ["joint_angles_rigid"]
    assert all(_same(plain[k], run[k]) for k in plain)
    assert run["points3d_rigid"].shape == (15, 38, 3) and run["rigid_segment_lengths"].shape == (6, 4)
    assert run["rigid_fit_cost"].shape == (15, 6) and run["joint_angles_rigid"].shape == (15, 6, 8)
    fit = ops.fit_legs(_dev(cuda, run["points3d_wo_procrustes"]))
    assert np.array_equal(run["points3d_rigid"], _host(fit.points)) and np.array_equal(run["rigid_fit_cost"], _host(fit.cost))
    assert np.array_equal(run["joint_angles_rigid"], _host(ops.joint_angles(fit.points)[0]))
    only = reopen("--rigid-legs")
    assert [str(k) for k in only.keys()] == [str(k) for k in g3["key_order"]] + RIGID_KEYS
    assert all(_same(plain[k], only[k]) for k in only if k in plain) and _same(only["points3d_rigid"], run["points3d_rigid"])
    config.pop("image_shape", None)
