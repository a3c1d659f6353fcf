"""CPU self-test of the pictorial-structures sweep's generators and comparators (tests/pictorial_compare.py), no device.

Every "device result" here is the float64 oracle's (tests/pictorial_oracle.py) with one mutation, on problems made by the
sweep's own generators.  The comparators must accept the oracle's own output and the same output with every U moved by one ulp
(what FMA contraction does), and must reject each simulated kernel bug on at least one generated problem: the evidence that
the sweep's inputs reach the places where those bugs would show."""
import numpy as np
import pytest

import pictorial_compare as pc
import pictorial_oracle as po

IMAGE_SHAPE = [960, 480]
K, T, M_ALL = 3, 3, 256
CASES = ("rev", "clc", "rand1")   # orderings of the generated problems (each with every edge switch on)


def _problems(golden_dir, nonfinite):
    P, g3 = pc.golden_cameras(golden_dir)
    out = {}
    for q, name in enumerate(CASES):
        order = pc.ORDERINGS[name]
        clean = pc.clean_points(g3, order, range(T))
        count, pts, vals = pc.make_problem(clean, order, K, seed=10 + q, zero_counts=True, bad_counts=True, zero_coords=True,
                                           duplicates=True, nonfinite=nonfinite)
        am = pc.argmax2d(pts, order)
        ora = po.proposals(P, order, am, count, pts, vals, IMAGE_SHAPE, K, M_ALL)
        out[name] = dict(P=P, order=order, count=count, pts=pts, vals=vals, am=am, all=ora["all"], kept=ora["kept"])
    return out


@pytest.fixture(scope="module")
def problems(golden_dir):
    """Every edge switch on."""
    return _problems(golden_dir, nonfinite=True)


@pytest.fixture(scope="module")
def finite_problems(golden_dir):
    """Every edge switch but the non-finite peak values on (with an infinite U in a chain, a frame's energy is NaN or infinite)."""
    return _problems(golden_dir, nonfinite=False)


def _kept_dev(all_rows, m, select=pc.select_kept, cap=None):
    return pc.kept_arrays([[select(o, m) for o in row] for row in all_rows], m, cap)


def _solve_setup(seed):
    from deepfly3d_amd.config import bone_tree

    parent, bone = bone_tree()
    rng = np.random.default_rng(seed)
    bone = np.stack([rng.uniform(0.2, 1.5, 38), rng.uniform(0.05, 0.6, 38)], axis=1)   # random mu / sigma on every joint
    return parent, bone


# ------------------------------------------------------------------------------------------------------------------ generators
def test_problem_generator_covers_the_edges(problems):
    for name, p in problems.items():
        count, pts, vals = p["count"], p["pts"], p["vals"]
        seen = np.zeros(count.shape, bool)
        for j, see in enumerate(po.seeing_table(p["order"])):
            for c, src, _ in see:
                seen[c, :, src] = True
        assert (count[seen] == 0).any() and (count[seen] > K).any() and (count[seen] < 0).any(), name
        assert (pts[seen][..., 0] == 0).any() and (pts[seen][..., 1] == 0).any(), name   # zero coordinates
        assert np.isnan(vals[seen]).any() and np.isinf(vals[seen]).any(), name
        dup = [(pl[0] == pl[1]).all() or (pl[0] == pl[2]).all() or (pl[1] == pl[2]).all() for pl in pts[seen]]
        assert any(dup), name
        # every frame has a joint that no seeing camera has a peak for
        for t in range(T):
            assert any(all(count[c, t, s] <= 0 for c, s, _ in see) for see in po.seeing_table(p["order"])), (name, t)
        # exact U ties between different kept proposals exist (duplicated pixels)
        ties = sum(len(o["U"]) - len(np.unique(o["U"])) for row in p["kept"] for o in row)
        assert ties > 0, name


def test_plane_generator_covers_the_edges():
    for h, w in [(64, 128), (8192, 1), (2, 4096), (128, 64)]:
        hm, kinds = pc.make_planes(h, w, 16, seed=3)
        count, _, vals = po.heatmap_peaks(hm[:, None], 16)
        for v in range(3):   # > 16 peaks in one lane, all of them above the rest of the plane
            p = hm[kinds.index("one_lane") + v]
            top = np.flatnonzero(p.reshape(-1) >= 2.0)
            assert len(top) > 16 and len(set(top % 64)) == 1, (h, w, v)
        ek = [i for i, n in enumerate(kinds) if n == "exact_k"]
        fk = [i for i, n in enumerate(kinds) if n == "fewer_k"]
        assert np.all(count[ek, 0] == 16) and np.all(count[fk, 0] < 16), (h, w)
        sub = hm[kinds.index("subnormal")]
        assert ((sub != 0) & (np.abs(sub) < np.finfo(np.float32).tiny)).mean() > 0.5
        sz = hm[kinds.index("signed_zero")]
        assert (np.signbit(sz) & (sz == 0)).any() and (~np.signbit(sz) & (sz == 0)).any()
    assert len(pc.legal_plane_shapes()) == 84 and all(64 <= h * w <= 8192 for h, w in pc.legal_plane_shapes())


# ------------------------------------------------------------------------------------------------------------------ accepted
@pytest.mark.parametrize("m", [1, 2, 3 * K * K + 1, 3 * K * K + 2, 256])
def test_kept_comparator_accepts_the_oracle(problems, m):
    for p in problems.values():
        rep = pc.compare_kept(_kept_dev(p["all"], m), p["all"], m)
        assert rep.ok, str(rep)


def _ulp_moved(all_rows):
    """Every U moved by one ulp up or down, the direction a function of U's bits (identical inputs round identically, as on the
    device), and the kept sets selected again on the moved U."""
    out = []
    for row in all_rows:
        r2 = []
        for o in row:
            U = o["U"].copy()
            bits = U.view(np.uint64)
            up = ((bits * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63)).astype(bool)
            fin = np.isfinite(U)
            U[fin & up] = np.nextafter(U[fin & up], np.inf)
            U[fin & ~up] = np.nextafter(U[fin & ~up], -np.inf)
            r2.append(dict(o, U=U))
        out.append(r2)
    return out


@pytest.mark.parametrize("m", [2, 3 * K * K + 1, 256])
def test_kept_comparator_accepts_one_ulp_in_u(problems, m):
    for p in problems.values():
        dev = _kept_dev(_ulp_moved(p["all"]), m)
        assert not np.array_equal(dev["U"], _kept_dev(p["all"], m)["U"])
        rep = pc.compare_kept(dev, p["all"], m)
        assert rep.ok, str(rep)


def test_solve_comparator_accepts_the_oracle(problems, finite_problems):
    for q, p in enumerate(list(problems.values()) + list(finite_problems.values())):
        parent, bone = _solve_setup(q)
        ora = po.solve(p["kept"], p["order"], p["am"], p["count"], p["pts"], parent, bone)
        assert pc.compare_solve(ora[:3], ora).ok
        e = ora[2].copy()
        e[np.isfinite(e)] = np.nextafter(e[np.isfinite(e)], np.inf)
        assert pc.compare_solve((ora[0], ora[1], e), ora).ok


def test_peak_comparator_accepts_the_oracle():
    hm, _ = pc.make_planes(8, 8, 7, seed=1)
    want = po.heatmap_peaks(hm[:, None], 7)
    assert pc.compare_peaks(tuple(x.copy() for x in want), want).ok


# ------------------------------------------------------------------------------------------------------------------ rejected
def _left_cameras(order):
    return [order[i] for i in (4, 5, 6)]


def _bug_proposals(p, bug, m):
    """The kept sets of a device with `bug`, and the m its comparator runs at."""
    P, order, am, count, pts, vals = (p[x] for x in ("P", "order", "am", "count", "pts", "vals"))
    if bug == "ordering_ignored":   # pos[c] = c
        return _kept_dev(po.proposals(P, pc.IDENTITY, am, count, pts, vals, IMAGE_SHAPE, K, M_ALL)["all"], m)
    if bug == "left_unflip_dropped":   # the proposals use the network's (flipped) columns of the left cameras
        p2 = pts.astype(np.float64)
        for c in _left_cameras(order):
            p2[c, ..., 1] = 1.0 - p2[c, ..., 1]
        return _kept_dev(po.proposals(P, order, am, count, p2, vals, IMAGE_SHAPE, K, M_ALL)["all"], m)
    if bug == "ties_to_higher_index":
        def sel(o, m):
            keep = np.concatenate([[0], np.lexsort((-o["index"][1:], o["U"][1:]))[: m - 1] + 1])
            return {n: o[n][keep] for n in ("index", "X", "U", "match")}
        return _kept_dev(p["all"], m, sel)
    if bug == "m_others_kept":
        def sel(o, m):
            return pc.select_kept(o, m + 1)
        return _kept_dev(p["all"], m, sel, cap=m + 1)
    if bug == "counts_unclamped":   # slots past K read the memory that follows: the next plane's peaks
        kx = 2 * K
        fp, fv = pts.reshape(-1, 2), vals.reshape(-1)
        pe = np.zeros(pts.shape[:3] + (kx, 2), np.float32)
        ve = np.zeros(vals.shape[:3] + (kx,), np.float32)
        for pl in range(count.size):
            c, t, s = np.unravel_index(pl, count.shape)
            n = min(fp.shape[0] - pl * K, kx)
            pe[c, t, s, :n] = fp[pl * K : pl * K + n]
            ve[c, t, s, :n] = fv[pl * K : pl * K + n]
        raw = np.minimum(count, kx)   # the device's count, unclamped (up to what this simulation extends)
        rows = po.proposals(P, order, am, raw, pe, ve, IMAGE_SHAPE, kx, M_ALL)["all"]
        for row in rows:   # the device numbers proposals with its own K
            for o in row:
                i = o["index"]
                q, r = (i - 1) // (kx * kx), (i - 1) % (kx * kx)
                o["index"] = np.where(i == 0, 0, 1 + q * K * K + (r // kx) * K + r % kx)
        return _kept_dev(rows, m)
    raise ValueError(bug)


PROPOSAL_BUGS = ["ordering_ignored", "left_unflip_dropped", "ties_to_higher_index", "m_others_kept", "counts_unclamped"]


@pytest.mark.parametrize("bug", PROPOSAL_BUGS)
def test_kept_comparator_rejects(problems, bug):
    rejected = []
    for name, p in problems.items():
        for m in (2, 3 * K * K + 1, 256):
            rep = pc.compare_kept(_bug_proposals(p, bug, m), p["all"], m)
            rejected.append(not rep.ok)
    assert any(rejected), bug


def test_kept_comparator_rejects_t0_ignored(problems):
    """A chunk [t0, t1) whose proposal 0 is read at frame t - t0 instead of t."""
    rejected = False
    for p in problems.values():
        t0 = 1
        am_shift = p["am"].copy()
        am_shift[:, t0:] = p["am"][:, : T - t0]
        rows = po.proposals(p["P"], p["order"], am_shift, p["count"], p["pts"], p["vals"], IMAGE_SHAPE, K, M_ALL)["all"][t0:]
        rep = pc.compare_kept(_kept_dev(rows, 64), p["all"], 64, frames=range(t0, T))
        assert pc.compare_kept(_kept_dev(p["all"][t0:], 64), p["all"], 64, frames=range(t0, T)).ok
        rejected |= not rep.ok
    assert rejected


def _solve_bug(p, bug, parent, bone):
    kept = p["kept"]
    args = (p["order"], p["am"], p["count"], p["pts"])
    if bug == "match_byte_by_camera":   # byte (8 c) mod 32 of the match word for physical camera c, not its rank among the seeing cameras
        table = po.seeing_table(p["order"])
        k2 = []
        for row in kept:
            r2 = []
            for j, o in enumerate(row):
                new = np.zeros_like(o["match"])
                for a, (c, _, _) in enumerate(table[j]):
                    new |= ((o["match"] >> ((8 * c) % 32)) & 0xFF) << (8 * a)
                r2.append(dict(o, match=new))
            k2.append(r2)
        return po.solve(k2, *args, parent, bone)
    if bug == "parent_sigma":   # the bone (parent, child) scaled by the parent's sigma
        b2 = bone.copy()
        for j, par in enumerate(parent):
            if par >= 0:
                b2[j, 1] = bone[par, 1]
        return po.solve(kept, *args, parent, b2)
    if bug == "slot_past_kcount":   # the solve reads one slot past kcount (attractive poison there)
        k2 = [[{n: np.concatenate([o[n], o[n][:1] * 0 + (-1e6 if n == "U" else 0)]) for n in ("index", "X", "U", "match")} for o in row] for row in kept]
        return po.solve(k2, *args, parent, bone)
    raise ValueError(bug)


@pytest.mark.parametrize("bug", ["match_byte_by_camera", "parent_sigma", "slot_past_kcount"])
def test_solve_comparator_rejects(finite_problems, bug):
    rejected = []
    for q, p in enumerate(finite_problems.values()):
        parent, bone = _solve_setup(q)
        ora = po.solve(p["kept"], p["order"], p["am"], p["count"], p["pts"], parent, bone)
        dev = _solve_bug(p, bug, parent, bone)
        rejected.append(not pc.compare_solve(dev[:3], ora).ok)
    assert any(rejected), bug


def _peaks_before_ge(hm, k):
    """po.heatmap_peaks with >= (not >) towards the neighbours before a cell in row-major order."""
    hm = np.asarray(hm, np.float32)
    n, J, H, W = hm.shape
    pad = np.full((n, J, H + 2, W + 2), np.nan, np.float32)
    pad[:, :, 1:-1, 1:-1] = hm
    peak = np.isfinite(hm)
    with np.errstate(invalid="ignore"):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if dr or dc:
                    q = pad[:, :, 1 + dr : 1 + dr + H, 1 + dc : 1 + dc + W]
                    peak &= (hm >= q) | ~np.isfinite(q)
    count = np.zeros((n, J), np.int32)
    pts = np.zeros((n, J, k, 2), np.float32)
    vals = np.zeros((n, J, k), np.float32)
    flat, pflat = hm.reshape(n, J, H * W), peak.reshape(n, J, H * W)
    for a in range(n):
        for b in range(J):
            idx = np.flatnonzero(pflat[a, b])
            sel = idx[np.lexsort((idx, -flat[a, b, idx]))][:k]
            count[a, b] = sel.size
            pts[a, b, : sel.size, 0] = (sel // W).astype(np.float32) * (np.float32(1) / np.float32(H))
            pts[a, b, : sel.size, 1] = (sel % W).astype(np.float32) * (np.float32(1) / np.float32(W))
            vals[a, b, : sel.size] = flat[a, b, sel]
    return count, pts, vals


def _ftz(hm):
    hm = hm.copy()
    sub = np.isfinite(hm) & (np.abs(hm) < np.finfo(np.float32).tiny)
    hm[sub] = np.copysign(np.float32(0), hm[sub])
    return hm


@pytest.mark.parametrize("bug", ["before_ge", "unused_slots_unwritten", "subnormals_flushed"])
def test_peak_comparator_rejects(bug):
    rejected = []
    for (h, w) in [(8, 8), (64, 128), (2, 4096)]:
        for k in (1, 7, 16):
            hm, _ = pc.make_planes(h, w, k, seed=h + k)
            hm = hm[:, None]
            want = po.heatmap_peaks(hm, k)
            if bug == "before_ge":
                got = _peaks_before_ge(hm, k)
            elif bug == "unused_slots_unwritten":
                c, pt, v = (x.copy() for x in want)
                unused = np.arange(k)[None, None] >= c[..., None]
                pt[unused] = np.nan
                v[unused] = np.nan
                got = (c, pt, v)
            else:
                got = po.heatmap_peaks(_ftz(hm), k)
            rejected.append(not pc.compare_peaks(got, want).ok)
    assert any(rejected), bug
