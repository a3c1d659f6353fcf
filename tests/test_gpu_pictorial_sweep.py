"""-m gpu: the pictorial-structures kernels (deepfly3d_amd/csrc/pictorial.hip) swept against the float64 oracle
(tests/pictorial_oracle.py) over camera orderings, K, M, image shapes, tau and weights, frame ranges, parent tables, plane shapes
and plane kinds, with the generators and comparators of tests/pictorial_compare.py.  Outputs are poisoned before the calls made
through the C entries: unused peak slots must be written, kept slots at or past kcount must be neither written nor read.

Bounds, with the worst value measured on the MI355X over the whole module:
    peaks (count, points, values, unused slots)   bit-identical                   (measured: 0 elements differ)
    peak 0 where the plane maximum is finite      bit-identical to the arg-max    (measured: 0 differ)
    kept count                                    exact                           (measured: exact)
    kept index order                              exact outside near-tie groups of oracle U (|dU| <= 1e-12 max(1, |U|)), exact
                                                  ties to the lower index        (measured: holds)
    kept U                                        1e-9 max(1, |U|)                (measured: 5.95e-12)
    kept X                                        1e-9 max(1, |X|)                (measured: 3.17e-11)
    kept match                                    exact                           (measured: exact)
    energy                                        1e-9 max(1, |E|)                (measured: 6.39e-14)
    choice                                        exact where the margin > 1e-9 max(1, |E|)   (measured: 0 choices differ,
                                                  inside the tolerance or out)
    points2d                                      bit-identical where the choices agree        (measured: 0 differ)
    chunked / tiled frame ranges                  bit-identical to one chunk / to frame 0      (measured: 0 differ)
The simulated bugs of tests/test_pictorial_compare.py fail these comparators on the same generators.  No kernel bug was found.
The module runs in about 30 seconds (the oracle dominates)."""
import ctypes

import numpy as np
import pytest
import torch

import pictorial_compare as pc
import pictorial_oracle as po

pytestmark = pytest.mark.gpu

IMAGE_SHAPES = ([960, 480], [1920, 960])   # [W, H]
NAN32 = 0x7FC0DEAD                          # a quiet-NaN bit pattern, also read as an int32
NAN64 = 0x7FF8DEADBEEFDEAD
WORST = {}


def _note(rep):
    for key, v in rep.worst.items():
        WORST[key] = max(WORST.get(key, 0.0), v)
    print("WORST", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


def _to(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _poisoned(shape, dtype, cuda):
    if dtype == torch.float64:
        return torch.full(shape, NAN64, dtype=torch.int64, device=cuda).view(torch.float64)
    return torch.full(shape, NAN32, dtype=torch.int32, device=cuda).view(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits_t(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------------------------ peaks
def _peaks_c(lib, hm, k, cuda):
    """df3d_heatmap_peaks through ctypes into NaN-poisoned outputs: hm [n, J, h, w] float32 numpy."""
    n, J, h, w = hm.shape
    d = _to(cuda, hm.astype(np.float32))[0]
    count = _poisoned((n, J), torch.int32, cuda)
    pts = _poisoned((n, J, k, 2), torch.float32, cuda)
    vals = _poisoned((n, J, k), torch.float32, cuda)
    rc = lib.df3d_heatmap_peaks(d.data_ptr(), n, J, h, w, k, count.data_ptr(), pts.data_ptr(), vals.data_ptr(), _stream())
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()
    return d, (count.cpu().numpy(), pts.cpu().numpy(), vals.cpu().numpy())


def _check_peaks(lib, hm, k, cuda):
    from deepfly3d_amd import ops

    d, got = _peaks_c(lib, hm, k, cuda)
    rep = pc.compare_peaks(got, po.heatmap_peaks(hm, k))
    # peak 0 is the arg-max cell wherever the plane's maximum is finite
    ap, ac = (x.cpu().numpy() for x in ops.heatmap_argmax(d))
    comparable = (got[0] > 0) & ~np.isposinf(hm).any(axis=(2, 3))
    bad = comparable & ((pc._bits(got[1][:, :, 0]) != pc._bits(ap)).any(-1) | (pc._bits(got[2][:, :, 0]) != pc._bits(ac)))
    for p in np.argwhere(bad)[:8]:
        rep.fail(f"plane {tuple(p)}: peak 0 {got[1][tuple(p)][0]} {got[2][tuple(p)][0]} != arg-max {ap[tuple(p)]} {ac[tuple(p)]}")
    _note(rep)
    assert rep.ok, str(rep)
    return got


PEAK_SHAPES = [(1, 64), (64, 1), (8, 8), (16, 32), (64, 128), (128, 64), (2, 4096), (8192, 1)]


@pytest.mark.parametrize("k", [1, 2, 7, 16])
@pytest.mark.parametrize("h,w", PEAK_SHAPES)
def test_peaks_every_kind(native_lib, cuda, h, w, k):
    hm, kinds = pc.make_planes(h, w, k, seed=h * 31 + w + k)
    got = _check_peaks(native_lib, hm.reshape(3, -1, h, w), k, cuda)
    count = got[0].reshape(-1)
    assert (count == k).any() and (count[np.array(kinds) == "fewer_k"] < k).all()


def test_peaks_every_legal_shape(native_lib, cuda):
    for h, w in pc.legal_plane_shapes():
        for k in (3, 16):
            hm, _ = pc.make_planes(h, w, k, seed=h + 7 * w + k, per_kind=1)
            _check_peaks(native_lib, hm[None], k, cuda)


def test_peaks_more_than_65536_planes(native_lib, cuda):
    rng = np.random.default_rng(9)
    hm = rng.integers(0, 4, size=(3500, 19, 8, 8)).astype(np.float32) + rng.random((3500, 19, 1, 1), dtype=np.float32)
    hm[rng.random(hm.shape) < 0.01] = np.nan
    _check_peaks(native_lib, hm, 7, cuda)


# ------------------------------------------------------------------------------------------------------------------ proposals
def _problem(golden_dir, order, k, T, seed, image_shape=IMAGE_SHAPES[0], nonfinite=True, frames=None):
    P, g3 = pc.golden_cameras(golden_dir)
    clean = pc.clean_points(g3, order, range(T) if frames is None else frames, image_shape)
    count, pts, vals = pc.make_problem(clean, order, k, seed, zero_counts=True, bad_counts=True, zero_coords=True, duplicates=True,
                                       nonfinite=nonfinite)
    return P, count, pts, vals


def _device_inputs(P, order, count, pts, vals, image_shape, cuda):
    from deepfly3d_amd import ops

    dc, dp, dv = _to(cuda, count, pts, vals)
    am = ops.relayout_19_to_38(dp[:, :, :, 0].contiguous(), order)
    assert np.array_equal(am.cpu().numpy(), pc.argmax2d(pts, order))
    X0 = ops.arg_max_points3d(P, am, image_shape)
    return am, X0, dc, dp, dv


def _proposals_c(lib, P, order, am, X0, dc, dp, dv, t0, tn, m, image_shape, tau, w_r, w_h, cuda):
    """df3d_ps_proposals through ctypes into NaN-poisoned kept buffers; slots at or past kcount must keep the poison."""
    T, k = am.shape[1], dp.shape[3]
    kept = {"count": _poisoned((tn, 38), torch.int32, cuda), "index": _poisoned((tn, 38, m), torch.int32, cuda),
            "X": _poisoned((tn, 38, m, 3), torch.float64, cuda), "U": _poisoned((tn, 38, m), torch.float64, cuda),
            "match": _poisoned((tn, 38, m), torch.int32, cuda)}
    Ph = np.ascontiguousarray(P, np.float64)
    rc = lib.df3d_ps_proposals(Ph.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), (ctypes.c_int * 7)(*order), X0.data_ptr(), dc.data_ptr(),
                               dp.data_ptr(), dv.data_ptr(), T, t0, tn, k, m, float(image_shape[1]), float(image_shape[0]), float(tau),
                               float(w_r), float(w_h), kept["count"].data_ptr(), kept["index"].data_ptr(), kept["X"].data_ptr(),
                               kept["U"].data_ptr(), kept["match"].data_ptr(), _stream())
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()
    cnt = kept["count"].long()
    unused = torch.arange(m, device=cuda)[None, None] >= cnt[..., None]
    for name in ("index", "U", "match"):
        b = _bits_t(kept[name])
        assert bool((b[unused] == (NAN64 if b.dtype == torch.int64 else NAN32)).all()), f"kept {name} written past kcount"
    assert bool((_bits_t(kept["X"])[unused] == NAN64).all()), "kept X written past kcount"
    return {n: t.cpu().numpy() for n, t in kept.items()}, kept


def _configs(k):
    out = [(img, tau, w) for img in range(2) for tau in (0.5, 30.0, 1e4) for w in ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0))]
    return out if k < 16 else out[::3]


@pytest.mark.parametrize("k,T", [(1, 4), (3, 3), (16, 1)])
@pytest.mark.parametrize("order_name", list(pc.ORDERINGS))
def test_proposals_sweep(native_lib, cuda, golden_dir, order_name, k, T):
    order = pc.ORDERINGS[order_name]
    for img_i, tau, (w_r, w_h) in _configs(k):
        image_shape = IMAGE_SHAPES[img_i]
        P, count, pts, vals = _problem(golden_dir, order, k, T, seed=k * 100 + img_i, image_shape=image_shape)
        am, X0, dc, dp, dv = _device_inputs(P, order, count, pts, vals, image_shape, cuda)
        ora = po.proposals(P, order, am.cpu().numpy(), count, pts, vals, image_shape, k, 256, tau, w_r, w_h)["all"]
        for m in sorted({1, 2, min(3 * k * k + 1, 255), min(3 * k * k + 2, 256), 256}):   # at K = 16, 3K^2 + 1 = 769 > 256
            dev, _ = _proposals_c(native_lib, P, order, am, X0, dc, dp, dv, 0, T, m, image_shape, tau, w_r, w_h, cuda)
            # proposal 0 is df3d_triangulate_scaled's point, bit for bit
            assert np.array_equal(pc._bits(dev["X"][:, :, 0]), pc._bits(X0.cpu().numpy())), (tau, w_r, w_h, m)
            rep = pc.compare_kept(dev, ora, m)
            _note(rep)
            assert rep.ok, f"{order_name} k={k} img={image_shape} tau={tau} w=({w_r}, {w_h}) m={m}: {rep}"
            if w_r == 0.0 and w_h == 0.0:   # every U is 0 (or +inf where a matched value is not finite): pure index order
                for t in range(T):
                    for j in range(38):
                        want = pc.select_kept(ora[t][j], m)["index"]
                        assert np.array_equal(dev["index"][t, j, : len(want)], want), (t, j, m)


# ------------------------------------------------------------------------------------------------------------------ frame ranges
def test_chunked_frames_equal_one_chunk(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import bone_tree

    order, k, T, m = pc.ORDERINGS["clc"], 3, 7, 16
    P, count, pts, vals = _problem(golden_dir, order, k, T, seed=5, nonfinite=False)
    am, X0, dc, dp, dv = _device_inputs(P, order, count, pts, vals, IMAGE_SHAPES[0], cuda)
    one = ops.ps_proposals(P, order, am, dc, dp, dv, IMAGE_SHAPES[0], num_proposals=m, X0=X0)
    one_out = [x.cpu().numpy() for x in ops.ps_solve(order, am, dc, dp, one)]
    one = {n: t.cpu().numpy() for n, t in one.items()}
    for chunk in (1, 2, 3):
        out = None
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            kept = ops.ps_proposals(P, order, am, dc, dp, dv, IMAGE_SHAPES[0], frames=(t0, t1), num_proposals=m, X0=X0)
            for n, t in kept.items():
                assert np.array_equal(pc._bits(t.cpu().numpy()), pc._bits(one[n][t0:t1])), (chunk, t0, n)
            out = ops.ps_solve(order, am, dc, dp, kept, frames=(t0, t1), out=out)
        for a, b in zip(out, one_out):
            assert np.array_equal(pc._bits(a.cpu().numpy()), pc._bits(b)), chunk
        res = ops.pictorial_correct(P, order, am, dc, dp, dv, IMAGE_SHAPES[0], num_proposals=m, chunk_frames=chunk)
        for a, b in zip((res.points2d, res.choice, res.energy), one_out):
            assert np.array_equal(pc._bits(a.cpu().numpy()), pc._bits(b)), chunk
    ora = po.proposals(P, order, am.cpu().numpy(), count, pts, vals, IMAGE_SHAPES[0], k, m)
    rep = pc.compare_kept(one, ora["all"], m)
    parent, bone = bone_tree()
    rep = pc.compare_solve(one_out, po.solve(ora["kept"], order, am.cpu().numpy(), count, pts, parent, bone), rep)
    _note(rep)
    assert rep.ok, str(rep)


def test_65535_tiled_frames_at_a_large_offset(native_lib, cuda, golden_dir):
    """One problem frame tiled to 65 540 frames; proposals and solve of frames [5, 65 540) in one call each (tn = 65 535, the
    limit): every frame bit-identical to the first, and that one to the oracle."""
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import bone_tree

    order, k, m, t0, tn = pc.ORDERINGS["rev"], 3, 8, 5, 65535
    T = t0 + tn
    P, count, pts, vals = _problem(golden_dir, order, k, 1, seed=77, nonfinite=False)
    d1 = _to(cuda, count, pts, vals)
    dc, dp, dv = (x.expand(7, T, *x.shape[2:]).contiguous() for x in d1)
    am = ops.relayout_19_to_38(dp[:, :, :, 0].contiguous(), order)
    X0 = ops.arg_max_points3d(P, am, IMAGE_SHAPES[0])
    kept = ops.ps_proposals(P, order, am, dc, dp, dv, IMAGE_SHAPES[0], frames=(t0, T), num_proposals=m, X0=X0)
    for n, t in kept.items():
        b = _bits_t(t)
        assert bool((b == b[:1]).all()), n
    out = ops.ps_solve(order, am, dc, dp, kept, frames=(t0, T))
    pts2, choice, energy = out
    for name, t in (("points2d", pts2[:, t0:]), ("choice", choice[t0:]), ("energy", energy[t0:])):
        b = _bits_t(t)
        ref = b[:, :1] if name == "points2d" else b[:1]
        assert bool((b == ref).all()), name
    assert bool((_bits_t(pts2[:, :t0]) == _bits_t(am[:, :t0])).all()) and bool((choice[:t0] == 0).all())   # frames before t0 untouched
    first = {n: t[:1].cpu().numpy() for n, t in kept.items()}
    del kept
    amh = am[:, :1].cpu().numpy()
    ora = po.proposals(P, order, amh, count, pts, vals, IMAGE_SHAPES[0], k, m)
    rep = pc.compare_kept(first, ora["all"], m)
    parent, bone = bone_tree()
    o = po.solve(ora["kept"], order, amh, count, pts, parent, bone)
    rep = pc.compare_solve((pts2[:, t0 : t0 + 1].cpu().numpy(), choice[t0 : t0 + 1].cpu().numpy(), energy[t0 : t0 + 1].cpu().numpy()), o, rep)
    _note(rep)
    assert rep.ok, str(rep)


# ------------------------------------------------------------------------------------------------------------------ solve
def _parent_tables():
    from deepfly3d_amd.config import bone_tree

    rng = np.random.default_rng(12)
    tables = {"bone_tree": bone_tree()[0]}
    perm = rng.permutation(38)
    chain = np.full(38, -1, np.int64)
    chain[perm[1:]] = perm[:-1]   # one 38-joint chain through the joints in a shuffled order
    tables["one_chain"] = chain
    tables["singles"] = np.full(38, -1, np.int64)
    mixed = np.full(38, -1, np.int64)   # chains of 1..6 joints, shuffled: roots neither first in joint order nor increasing
    perm, at = rng.permutation(38), 0
    while at < 38:
        n = int(rng.integers(1, 7))
        seg = perm[at : at + n]
        mixed[seg[1:]] = seg[:-1]
        at += n
    tables["short_chains"] = mixed
    return tables


def _solve_c(lib, order, parent, bone, w_b, am, dc, dp, kept, k, m, cuda):
    T = am.shape[1]
    out = am.clone()
    choice = torch.full((T, 38), -99, dtype=torch.int32, device=cuda)
    energy = _poisoned((T,), torch.float64, cuda)
    work = torch.empty((38 * T,), dtype=torch.float64, device=cuda)
    rc = lib.df3d_ps_solve((ctypes.c_int * 7)(*order), (ctypes.c_int * 38)(*[int(p) for p in parent]),
                           (ctypes.c_double * 76)(*np.asarray(bone, np.float64).reshape(-1)), float(w_b), am.data_ptr(), dc.data_ptr(),
                           dp.data_ptr(), T, 0, T, k, m, kept["count"].data_ptr(), kept["index"].data_ptr(), kept["X"].data_ptr(),
                           kept["U"].data_ptr(), kept["match"].data_ptr(), out.data_ptr(), choice.data_ptr(), energy.data_ptr(),
                           work.data_ptr(), work.numel(), _stream())
    assert rc == 0, lib.df3d_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), choice.cpu().numpy(), energy.cpu().numpy()


def _synthetic_kept(rng, T, m):
    """Kept sets as any caller of the C entry may pass them: counts 1..m (some 0 or above m: clamped), random proposals with
    exact ties in U and repeated points."""
    cnt = rng.integers(1, m + 1, size=(T, 38)).astype(np.int32)
    cnt[rng.random((T, 38)) < 0.1] = m
    cnt[rng.random((T, 38)) < 0.05] = 0
    cnt[rng.random((T, 38)) < 0.05] = m + 3
    index = np.stack([np.stack([rng.permutation(3 * 16 * 16 + 1)[:m] for _ in range(38)]) for _ in range(T)]).astype(np.int32)
    index[:, :, 0] = 0
    X = rng.normal(0, 0.6, size=(T, 38, m, 3))
    U = rng.normal(0, 1, size=(T, 38, m))
    if m >= 4:
        U[:, :, 3] = U[:, :, 2]
        X[:, :, 1] = X[:, :, 0]
    match = rng.integers(0, 1 << 24, size=(T, 38, m)).astype(np.int32)
    return {"count": cnt, "index": index, "X": X, "U": U, "match": match}


SOLVE_TABLES = ["bone_tree", "one_chain", "singles", "short_chains"]


@pytest.mark.parametrize("table", SOLVE_TABLES)
def test_solve_parent_tables(native_lib, cuda, table):
    order_names = list(pc.ORDERINGS)
    parent = _parent_tables()[table]
    rng = np.random.default_rng(40 + SOLVE_TABLES.index(table))
    T, k = 2, 4
    for q, m in enumerate((1, 2, 3, 17, 256)):
        order = pc.ORDERINGS[order_names[q % len(order_names)]]
        bone = np.stack([rng.uniform(0.2, 1.5, 38), rng.uniform(0.05, 0.6, 38)], axis=1)
        kept = _synthetic_kept(rng, T, m)
        count = rng.integers(-2, 7, size=(7, T, 19)).astype(np.int32)
        pts = (rng.integers(0, 64, size=(7, T, 19, k, 2)) / 64).astype(np.float32)
        am = rng.random((7, T, 38, 2))
        dam, dc, dp = _to(cuda, am, count, pts)
        for w_b in (0.0, 1.0, 1e3):
            ref = None
            for poison in ("none", "nan", "attractive"):
                dk = {n: _to(cuda, a)[0] for n, a in kept.items()}
                unused = torch.arange(m, device=cuda)[None, None] >= dk["count"].clamp(1, m).long()[..., None]
                if poison == "nan":
                    for n in ("X", "U"):
                        dk[n][unused] = float("nan")
                    dk["index"][unused], dk["match"][unused] = NAN32, NAN32
                elif poison == "attractive":   # a slot the solve must not read: far better than any real one
                    dk["U"][unused] = -1e6
                    dk["X"][unused] = 0.0
                    dk["index"][unused], dk["match"][unused] = -7, 0
                got = _solve_c(native_lib, order, parent, bone, w_b, dam, dc, dp, dk, k, m, cuda)
                if ref is None:
                    ref = got
                else:
                    for a, b in zip(got, ref):
                        assert np.array_equal(pc._bits(a), pc._bits(b)), (table, m, w_b, poison)
            o = po.solve(pc.kept_lists(kept), order, am, count, pts, parent, bone, w_b, k)
            rep = pc.compare_solve(ref, o)
            if m <= 3:   # brute force on the chains of up to 6 joints
                lists = pc.kept_lists(kept)
                for ch in po.chains_from_parent(parent):
                    if len(ch) > 6:
                        continue
                    for t in range(T):
                        U = [lists[t][j]["U"] for j in ch]
                        X = [lists[t][j]["X"] for j in ch]
                        e, sel = po.chain_brute(U, X, [bone[j][0] for j in ch], [bone[j][1] if parent[j] >= 0 else 1.0 for j in ch], w_b)
                        e_dp, sel_dp = po.chain_dp(U, X, [bone[j][0] for j in ch], [bone[j][1] if parent[j] >= 0 else 1.0 for j in ch], w_b)
                        assert abs(e - e_dp) <= 1e-12 * max(1.0, abs(e)), (table, ch)
                        clear = all(o[3][t, j] > pc.TOL * max(1.0, abs(o[2][t])) for j in ch)
                        if clear:
                            assert [int(ref[1][t, j]) for j in ch] == [int(lists[t][j]["index"][s]) for j, s in zip(ch, sel)], (table, ch, t)
            _note(rep)
            assert rep.ok, f"{table} m={m} w_b={w_b}: {rep}"


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("order_name", ["rev", "clc"])
def test_pictorial_correct_under_rig_orderings(native_lib, cuda, golden_dir, order_name):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import bone_tree

    order, k, T, m = pc.ORDERINGS[order_name], 10, 3, 64
    P, count, pts, vals = _problem(golden_dir, order, k, T, seed=31, nonfinite=False)
    am, X0, dc, dp, dv = _device_inputs(P, order, count, pts, vals, IMAGE_SHAPES[0], cuda)
    res = ops.pictorial_correct(P, order, am, dc, dp, dv, IMAGE_SHAPES[0], num_proposals=m)
    amh = am.cpu().numpy()
    ora = po.proposals(P, order, amh, count, pts, vals, IMAGE_SHAPES[0], k, m)
    parent, bone = bone_tree()
    o = po.solve(ora["kept"], order, amh, count, pts, parent, bone)
    rep = pc.compare_solve((res.points2d.cpu().numpy(), res.choice.cpu().numpy(), res.energy.cpu().numpy()), o)
    _note(rep)
    assert rep.ok, str(rep)
    assert (o[3] > 1e-9).mean() > 0.5
    assert (res.points2d.cpu().numpy() != amh).any()   # the correction moved something
