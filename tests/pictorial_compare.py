"""Generators and comparators of the pictorial-structures sweep (tests/test_gpu_pictorial_sweep.py) and of its CPU self-test
(tests/test_pictorial_compare.py).  Test infrastructure only (not collected: no test_ prefix); numpy and the float64 oracle
tests/pictorial_oracle.py.

Generators: `make_problem` scatters peaks around the projected golden pose for any camera ordering, with switches for the edges
(empty and out-of-range counts, zero coordinates, duplicated pixels, non-finite values); `make_planes` builds heat-map planes of
every kind the peaks kernel must get right.  Comparators return a `Report`: every difference at once, plus the worst error of
each kind, so that a test can both assert and print."""
import numpy as np

import pictorial_oracle as po

NJ, NPRED = po.NJ, po.NPRED
HM_H, HM_W = 64, 128   # the network's heat-map grid: peak points are multiples of 1 / 64 and 1 / 128

IDENTITY = [0, 1, 2, 3, 4, 5, 6]
ORDERINGS = {   # the identity, the two rig orderings of core._KNOWN_ORDERINGS and two seeded random permutations
    "identity": IDENTITY,
    "rev": [6, 5, 4, 3, 2, 1, 0],
    "clc": [0, 6, 5, 4, 3, 2, 1],
    "rand1": [int(c) for c in np.random.default_rng(101).permutation(7)],
    "rand2": [int(c) for c in np.random.default_rng(202).permutation(7)],
}

TOL = 1e-9        # relative tolerance of U, X and the energy: the kernels are float64 with FMA contraction, the oracle is numpy
TIE = 1e-12       # oracle U closer than TIE * max(1, |U|) form a near-tie group, whose order FMA rounding may permute


# ------------------------------------------------------------------------------------------------------------------ problems
def golden_cameras(golden_dir):
    from oracle import geometry as og

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    return og.projection_matrices(g3["R"], g3["tvec"], g3["intr"]), g3


def clean_points(g3, order, frames, image_shape=(960, 480)):
    """The golden pose of `frames` projected through the golden cameras, re-laid out for `order`: [7, T, 38, 2] normalised."""
    from deepfly3d_amd.synthetic import synthetic_points2d

    X = g3["points3d_wo_procrustes"][np.asarray(frames) % g3["points3d_wo_procrustes"].shape[0]]
    return synthetic_points2d(X, g3["R"], g3["tvec"], g3["intr"], camera_ordering=tuple(order), image_shape=tuple(image_shape))


def make_problem(clean, order, k, seed, zero_counts=False, bad_counts=False, zero_coords=False, duplicates=False, nonfinite=False):
    """Peaks of the network's planes (network orientation: left cameras flipped) scattered around `clean` ([7, T, 38, 2], the
    re-layout of `order`).  Returns count [7, T, 19] int32, pts [7, T, 19, k, 2] float32 (row / 64, col / 128), vals [7, T, 19, k]
    float32.  All k slots hold points even past the count, so that a kernel reading past it sees plausible peaks.
      zero_counts   some planes get count 0; on every frame one joint gets count 0 on all its seeing cameras
      bad_counts    some counts above k (up to k + 100) or below 0: the kernels clamp them to [0, k]
      zero_coords   some peaks in row 0 or column 0: a zero pixel coordinate drops that view from the DLT
      duplicates    some planes repeat a peak pixel: proposals built on the two copies tie exactly, the lower index wins
      nonfinite     some peak values are NaN or +-inf
    """
    T = clean.shape[1]
    rng = np.random.default_rng(seed)
    table = po.seeing_table(order)
    count = np.zeros((7, T, NPRED), np.int32)
    pts = np.zeros((7, T, NPRED, k, 2), np.float32)
    vals = np.zeros((7, T, NPRED, k), np.float32)
    lo = 0 if zero_coords else 1
    for j in range(NJ):
        for c, src, left in table[j]:
            for t in range(T):
                r0 = clean[c, t, j, 0] * HM_H
                c0 = (1.0 - clean[c, t, j, 1] if left else clean[c, t, j, 1]) * HM_W
                jitter = np.arange(k) > 0
                rr = np.clip(np.round(r0 + rng.normal(0, 4, k) * jitter), lo, HM_H - 1)
                cc = np.clip(np.round(c0 + rng.normal(0, 8, k) * jitter), lo, HM_W - 1)
                v = np.sort(rng.uniform(0.2, 1.0, k))[::-1].astype(np.float32)
                n = int(rng.integers(1, k + 1))
                if duplicates and k >= 2 and rng.random() < 0.5:
                    a, b = sorted(rng.choice(min(n, k) if n >= 2 else 2, size=2, replace=False))
                    rr[b], cc[b] = rr[a], cc[a]
                if zero_coords and rng.random() < 0.2:
                    s = int(rng.integers(0, n))
                    if rng.random() < 0.5:
                        rr[s] = 0
                    else:
                        cc[s] = 0
                if nonfinite and rng.random() < 0.15:
                    v[int(rng.integers(0, n))] = rng.choice([np.nan, np.inf, -np.inf])
                if zero_counts and rng.random() < 0.1:
                    n = 0
                if bad_counts and rng.random() < 0.2:
                    n = int(rng.integers(k + 1, k + 101)) if rng.random() < 0.5 else -int(rng.integers(1, 6))
                count[c, t, src] = n
                pts[c, t, src, :, 0] = rr.astype(np.float32) * np.float32(1 / HM_H)
                pts[c, t, src, :, 1] = cc.astype(np.float32) * np.float32(1 / HM_W)
                vals[c, t, src] = v
    if zero_counts:
        for t in range(T):
            j = int(rng.integers(NJ))
            for c, src, _ in table[j]:
                count[c, t, src] = 0
    return count, pts, vals


def argmax2d(pts, order):
    """The re-layout of the arg-max detections (peak 0 of every plane): [7, T, 38, 2] float64."""
    return po.og.relayout_19_to_38(pts[:, :, :, 0], list(order))


def kept_arrays(kept, m, cap=None):
    """The oracle's kept sets as the device lays them out: count [T, 38], index [T, 38, cap], X [.., 3], U, match (cap = m)."""
    T, cap = len(kept), m if cap is None else cap
    out = {"count": np.zeros((T, NJ), np.int32), "index": np.zeros((T, NJ, cap), np.int32), "X": np.zeros((T, NJ, cap, 3)),
           "U": np.zeros((T, NJ, cap)), "match": np.zeros((T, NJ, cap), np.int32)}
    for t in range(T):
        for j in range(NJ):
            o = kept[t][j]
            n = min(len(o["index"]), cap)
            out["count"][t, j] = n
            for name in ("index", "X", "U", "match"):
                out[name][t, j, :n] = o[name][:n]
    return out


def kept_lists(arrays):
    """Device kept arrays -> the oracle's [T][38] dict layout (the first `count` slots), for po.solve on the device's kept sets."""
    T = arrays["count"].shape[0]
    m = arrays["index"].shape[2]
    res = []
    for t in range(T):
        row = []
        for j in range(NJ):
            n = int(min(max(arrays["count"][t, j], 1), m))
            row.append({name: np.array(arrays[name][t, j, :n]) for name in ("index", "X", "U", "match")})
        res.append(row)
    return res


def select_kept(all_row, m):
    """The kept set of one (frame, joint) from all its proposals: proposal 0, then the m - 1 lowest (U, index)."""
    idx, U = all_row["index"], all_row["U"]
    keep = np.concatenate([[0], np.lexsort((idx[1:], U[1:]))[: m - 1] + 1]).astype(np.int64)
    return {name: all_row[name][keep] for name in ("index", "X", "U", "match")}


# ------------------------------------------------------------------------------------------------------------------ planes
PLANE_KINDS = ("noise", "plateau", "lane_ties", "one_lane", "exact_k", "fewer_k", "signed_zero", "subnormal", "nonfinite")


def _isolated(cells, h, w, rng=None, limit=None):
    """A subset of the flat `cells` (in the given order, shuffled when rng is given) no two of which are 8-neighbours."""
    cells = list(cells)
    if rng is not None:
        cells = list(rng.permutation(cells))
    taken, out = set(), []
    for p in cells:
        if limit is not None and len(out) == limit:
            break
        r, c = divmod(int(p), w)
        if any((r + dr, c + dc) in taken for dr in (-1, 0, 1) for dc in (-1, 0, 1)):
            continue
        taken.add((r, c))
        out.append(int(p))
    return out


def make_plane(kind, h, w, k, rng, variant=0):
    """One float32 heat-map plane [h, w] of the given kind:
      noise        standard normal
      plateau      values in {0, 1, 2} (plateaus, ties everywhere) and a flat-topped block
      lane_ties    noise in [0, 1) with isolated cells of equal value spread over many lanes
      one_lane     noise in [0, 1) and every isolated cell p = L (mod 64) of one lane L above all of it: more than 16 candidates in
                   one lane's register list wherever the plane has the cells (variant 0 random values, 1 increasing with p,
                   2 all equal)
      exact_k      exactly k finite cells (isolated) in a -inf (even variants) / NaN (odd) background: exactly k peaks
      fewer_k      the same with fewer than k (none for k = 1)
      signed_zero  +0, -0 and -1 cells
      subnormal    random float32 subnormals of both signs and zeros
      nonfinite    noise with NaN, +inf and -inf cells
    """
    hw = h * w
    if kind == "noise":
        return rng.standard_normal((h, w)).astype(np.float32)
    if kind == "plateau":
        p = rng.integers(0, 3, size=(h, w)).astype(np.float32)
        p[: max(1, h // 4), : max(1, w // 4)] = 3.0
        return p
    if kind == "lane_ties":
        p = rng.random((h, w)).astype(np.float32)
        flat = p.reshape(-1)
        for q, p_ in enumerate(_isolated(range(hw), h, w, rng, limit=24)):
            flat[p_] = 2.0 if q % 3 else 1.5
        return p
    if kind == "one_lane":
        p = rng.random((h, w)).astype(np.float32)
        flat = p.reshape(-1)
        lane = int(rng.integers(64))
        cells = _isolated(range(lane, hw, 64), h, w)
        if variant == 0:
            v = 2.0 + rng.random(len(cells))
        elif variant == 1:
            v = 2.0 + 0.01 * np.arange(len(cells))
        else:
            v = np.full(len(cells), 2.5)
        flat[cells] = v.astype(np.float32)
        return p
    if kind in ("exact_k", "fewer_k"):
        n = k if kind == "exact_k" else int(rng.integers(0, k))
        p = np.full(hw, -np.inf if variant % 2 == 0 else np.nan, np.float32)
        packing = _isolated(range(hw), h, w)   # row-major greedy: every other row and column, >= 16 cells in every legal shape
        cells = rng.choice(packing, size=n, replace=False)
        p[cells] = np.round(rng.random(len(cells)) * 4).astype(np.float32)   # coarse: equal values between peaks
        return p.reshape(h, w)
    if kind == "signed_zero":
        return rng.choice(np.array([0.0, -0.0, -1.0], np.float32), size=(h, w), p=[0.4, 0.4, 0.2])
    if kind == "subnormal":
        bits = rng.integers(0, 1 << 23, size=hw, dtype=np.uint32) | (rng.integers(0, 2, size=hw, dtype=np.uint32) << 31)
        bits[rng.random(hw) < 0.1] = 0
        return bits.view(np.float32).reshape(h, w)
    if kind == "nonfinite":
        p = rng.standard_normal((h, w)).astype(np.float32)
        u = rng.random((h, w))
        p[u < 0.05] = np.nan
        p[(u >= 0.05) & (u < 0.07)] = np.inf
        p[(u >= 0.07) & (u < 0.09)] = -np.inf
        return p
    raise ValueError(kind)


def make_planes(h, w, k, seed, kinds=PLANE_KINDS, per_kind=3):
    """[n, h, w] float32: `per_kind` planes (variants 0, 1, ...) of every kind, and the kind of each plane."""
    rng = np.random.default_rng(seed)
    planes, names = [], []
    for kind in kinds:
        for v in range(per_kind):
            planes.append(make_plane(kind, h, w, k, rng, v))
            names.append(kind)
    return np.stack(planes), names


def legal_plane_shapes():
    """Every (h, w) the peaks entry accepts: powers of two with 64 <= h * w <= 8192."""
    return [(1 << a, 1 << (s - a)) for s in range(6, 14) for a in range(s + 1)]


# ------------------------------------------------------------------------------------------------------------------ comparators
class Report:
    """Every difference a comparator found (`errors`) and the worst value of each measured error (`worst`)."""

    def __init__(self):
        self.errors, self.worst = [], {}

    def fail(self, msg):
        self.errors.append(msg)

    def see(self, name, value):
        value = float(value)
        if not np.isnan(value):
            self.worst[name] = max(self.worst.get(name, 0.0), value)

    @property
    def ok(self):
        return not self.errors

    def __str__(self):
        head = "; ".join(self.errors[:12])
        more = f" (+{len(self.errors) - 12} more)" if len(self.errors) > 12 else ""
        return f"{len(self.errors)} differences: {head}{more}; worst {self.worst}"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def compare_peaks(got, want, report=None):
    """Peaks (count, pts, vals) bit for bit: counts exact, every slot of pts and vals (the unused ones included, which must be
    zero) identical in its bits -- so NaN equals only the same NaN and -0 differs from +0."""
    rep = Report() if report is None else report
    gc, gp, gv = (np.asarray(x) for x in got)
    wc, wp, wv = (np.asarray(x) for x in want)
    if gc.shape != wc.shape or gp.shape != wp.shape or gv.shape != wv.shape:
        rep.fail(f"shapes {gc.shape, gp.shape, gv.shape} != {wc.shape, wp.shape, wv.shape}")
        return rep
    bad = np.argwhere(gc != wc)
    for p in bad[:8]:
        rep.fail(f"count{tuple(p)} {gc[tuple(p)]} != {wc[tuple(p)]}")
    if len(bad) > 8:
        rep.fail(f"... {len(bad)} planes with another count")
    for name, g, w in (("pts", gp, wp), ("vals", gv, wv)):
        diff = _bits(g.astype(np.float32)) != _bits(w.astype(np.float32))
        bad = np.argwhere(diff)
        for p in bad[:8]:
            rep.fail(f"{name}{tuple(p)} {g[tuple(p)]!r} != {w[tuple(p)]!r}")
        if len(bad) > 8:
            rep.fail(f"... {len(bad)} {name} elements differ")
        rep.see(f"{name}_elements_differing", len(bad))
    rep.see("count_planes_differing", int((gc != wc).sum()))
    return rep


def _close(got, want, tol):
    """|got - want| <= tol * max(1, |want|) elementwise; non-finite values must be equal (NaN to NaN)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - want) / np.maximum(1.0, np.abs(want)), 0.0)
    ok = np.where(fin, err <= tol, (got == want) | (np.isnan(got) & np.isnan(want)))
    return ok, np.where(np.isfinite(err), err, np.inf)


def compare_kept(dev, ora_all, m, report=None, frames=None):
    """Kept sets of the device (count [T, 38], index / U / match [T, 38, >= m], X [T, 38, >= m, 3], numpy) against the oracle's
    proposals (`po.proposals(...)["all"]`, one row per device frame; `frames` maps device frame -> oracle row, default equal).
    Per (t, j):
      - the count is exact, slot 0 is proposal 0;
      - the oracle's order (U, then index) is split into near-tie groups: runs of U within TIE * max(1, |U|) of each other.  The
        device's slots of a group hold the same indices as the oracle's (any order); the group at the M-th boundary may keep any
        of its members.  Outside near-tie groups this is exact equality;
      - exact ties (bit-identical oracle U: proposals of identical inputs) go to the lower index, in the kept set and in its order;
      - the device's own sequence is sorted by (its U, index);
      - U and X within TOL * max(1, |.|) of the oracle entry of the same index, match exactly."""
    rep = Report() if report is None else report
    T = dev["count"].shape[0]
    frames = list(range(T)) if frames is None else list(frames)
    for tl in range(T):
        for j in range(NJ):
            _compare_kept_one(rep, f"(t={tl}, j={j})", {n: dev[n][tl, j] for n in ("index", "X", "U", "match")}, int(dev["count"][tl, j]),
                              ora_all[frames[tl]][j], m)
    return rep


def _compare_kept_one(rep, where, dev, n_d, o, m):
    idx_o, U_o = o["index"], o["U"]
    others = np.lexsort((idx_o[1:], U_o[1:])) + 1
    n_o = 1 + min(len(others), m - 1)
    if n_d != n_o:
        rep.fail(f"{where} count {n_d} != {n_o}")
        return
    di = np.asarray(dev["index"][:n_d]).astype(np.int64)
    dU = np.asarray(dev["U"][:n_d], np.float64)
    if di[0] != 0:
        rep.fail(f"{where} slot 0 holds proposal {di[0]}")
    # near-tie groups of the oracle order (others[s] at slot 1 + s)
    Us = U_o[others]
    with np.errstate(invalid="ignore"):
        near = (Us[1:] == Us[:-1]) | (np.isfinite(Us[1:]) & np.isfinite(Us[:-1]) & (np.abs(Us[1:] - Us[:-1]) <= TIE * np.maximum(1.0, np.abs(Us[:-1]))))
    group = np.concatenate([[0], np.cumsum(~near)]).astype(np.int64)
    size = np.bincount(group) if len(group) else np.zeros(0, np.int64)
    w = n_o - 1
    o_ids, d_ids = idx_o[others[:w]], di[1:n_o]
    single = size[group[:w]] == 1
    for s in np.flatnonzero(single & (o_ids != d_ids))[:6]:
        rep.fail(f"{where} slot {1 + s} holds proposal {d_ids[s]}, oracle {o_ids[s]}")
    for g in np.unique(group[:w][~single]):
        members = np.flatnonzero(group == g)
        lo, hi = members[0], members[-1] + 1
        dev_g = d_ids[lo : min(hi, w)]
        g_ids = idx_o[others[lo:hi]]
        if len(set(dev_g.tolist())) != len(dev_g) or not set(dev_g.tolist()) <= set(g_ids.tolist()):
            rep.fail(f"{where} slots {1 + lo}..{min(hi, w)} hold {dev_g[:6].tolist()}, oracle near-tie group {g_ids[:6].tolist()}")
            continue
        if hi <= w and set(dev_g.tolist()) != set(g_ids.tolist()):
            rep.fail(f"{where} near-tie group at slot {1 + lo} differs")
        # exact ties (bit-identical oracle U): a kept member's peers of lower index are kept too, and come before it
        ubits = dict(zip(g_ids.tolist(), _bits(U_o[others[lo:hi]]).tolist()))
        for s, x in enumerate(dev_g.tolist()):
            for y in g_ids.tolist():
                if y < x and ubits[y] == ubits[x]:
                    at = np.flatnonzero(dev_g == y)
                    if not len(at):
                        rep.fail(f"{where} keeps {x} but not {y}, an exact tie of lower index")
                    elif at[0] > s:
                        rep.fail(f"{where} exact tie {y} placed after {x}")
    # the device's own order: (U, index) increasing over slots 1 ..
    if n_d > 2:
        a_u, b_u, a_i, b_i = dU[1:-1], dU[2:], di[1:-1], di[2:]
        bad = ~((a_u < b_u) | ((a_u == b_u) & (a_i < b_i)))
        for s in np.flatnonzero(bad)[:4]:
            rep.fail(f"{where} slots {s + 1}, {s + 2}: (U, index) ({a_u[s]!r}, {a_i[s]}) then ({b_u[s]!r}, {b_i[s]}) out of order")
    # values of every kept entry, against the oracle entry of the same index
    lookup = np.full(max(int(idx_o.max()), int(di.max()), 0) + 1, -1, np.int64)
    lookup[idx_o] = np.arange(len(idx_o))
    p = np.where(di >= 0, lookup[np.clip(di, 0, None)], -1)
    for s in np.flatnonzero(p < 0)[:4]:
        rep.fail(f"{where} slot {s} holds {di[s]}, not a proposal")
    ok = p >= 0
    s_ok, p_ok = np.flatnonzero(ok), p[ok]
    okU, eU = _close(dU[s_ok], U_o[p_ok], TOL)
    okX, eX = _close(np.asarray(dev["X"][:n_d])[s_ok], o["X"][p_ok], TOL)
    okM = np.asarray(dev["match"][:n_d])[s_ok].astype(np.int64) == o["match"][p_ok]
    if len(s_ok):
        rep.see("U_rel", eU.max())
        rep.see("X_rel", eX.max())
    for q in np.flatnonzero(~okU)[:4]:
        rep.fail(f"{where} slot {s_ok[q]} (proposal {di[s_ok[q]]}) U {dU[s_ok[q]]!r} != {U_o[p_ok[q]]!r}")
    for q in np.flatnonzero(~okX.all(axis=-1))[:4]:
        rep.fail(f"{where} slot {s_ok[q]} (proposal {di[s_ok[q]]}) X {dev['X'][s_ok[q]]} != {o['X'][p_ok[q]]}")
    for q in np.flatnonzero(~okM)[:4]:
        rep.fail(f"{where} slot {s_ok[q]} (proposal {di[s_ok[q]]}) match {int(dev['match'][s_ok[q]]):#x} != {int(o['match'][p_ok[q]]):#x}")


def compare_solve(dev, ora, report=None, tol=TOL):
    """The solve: dev = (points2d [7, T, 38, 2], choice [T, 38], energy [T]), ora = po.solve(...) (points2d, choice, energy,
    margin).  Energy within tol relative; the choice exact wherever the oracle's margin exceeds tol * max(1, |energy|); points2d
    bit for bit wherever the choices agree (every camera of that joint)."""
    rep = Report() if report is None else report
    d_pts, d_ch, d_e = (np.asarray(x) for x in dev)
    o_pts, o_ch, o_e, margin = (np.asarray(x) for x in ora)
    ok, err = _close(d_e, o_e, tol)
    rep.see("energy_rel", np.max(err) if err.size else 0.0)
    for t in np.flatnonzero(~ok)[:8]:
        rep.fail(f"energy[{t}] {d_e[t]!r} != {o_e[t]!r}")
    clear = margin > tol * np.maximum(1.0, np.abs(o_e))[:, None]
    bad = np.argwhere(clear & (d_ch != o_ch))
    for t, j in bad[:8]:
        rep.fail(f"choice[{t}, {j}] {d_ch[t, j]} != {o_ch[t, j]} (margin {margin[t, j]:.3g})")
    if len(bad) > 8:
        rep.fail(f"... {len(bad)} clear choices differ")
    same = d_ch == o_ch
    diff = (_bits(d_pts.astype(np.float64)) != _bits(o_pts.astype(np.float64))).any(axis=-1)   # [7, T, 38]
    bad = np.argwhere(diff & same[None])
    for c, t, j in bad[:8]:
        rep.fail(f"points2d[{c}, {t}, {j}] {d_pts[c, t, j]} != {o_pts[c, t, j]}")
    if len(bad) > 8:
        rep.fail(f"... {len(bad)} points differ where the choices agree")
    rep.see("choice_flips_within_tolerance", int((~same).sum()))
    return rep
