"""CPU certificate of the families tests/test_gpu_heatmap3d_sweep.py runs on the device (tests/heatmap3d_cases.py, DESIGN.md section 25,
"swept"): each family does what its name says, every search a GPU test asserts exactly is firm at every level -- its two best scores lie
further apart than GAP, or its best score is shared by points that are the same computation on the same numbers -- the window model
gives the cell counts the route tests rest on, and all of it takes a few seconds.  The oracle alone; nothing here touches a device."""
import time

import numpy as np
import pytest

import heatmap3d_cases as hc
import heatmap3d_oracle as ho

NEW = [name for names in hc.FAMILIES.values() for name in names]


def _searched(ref):
    return ref["status"] % 2 == 1


@pytest.mark.parametrize("name", NEW)
def test_every_new_case_is_firm(name):
    c, ref = hc.sweep(name), hc.sweep_reference(name)
    ok, searched = hc.firm(c, ref), _searched(ref)
    skipped = int((searched & ~ok).sum())
    print(f"{name}: hm {c['hm'].shape}, {int(searched.sum())} searched, {skipped} not firm, smallest gap_next {ref['gap_next'].min():.2e}, "
          f"{int((ref['ties'] >= 2).sum())} tied levels, statuses {np.bincount(ref['status'].ravel(), minlength=4).tolist()}")
    assert skipped <= hc.MAX_SKIPPED * ref["status"].size and hc.MAX_SKIPPED == 0.01 and hc.GAP == 1e-9
    if name in hc.NONE_LEFT_OUT:
        assert skipped == 0
    # the extra keys say what they say, and the old ones are what they were
    lv = ref["choice"] >= 0
    assert np.array_equal(ref["ties"] >= 1, lv) and np.array_equal(np.isfinite(ref["gap"]), lv)
    assert np.array_equal(ref["gap"] == 0.0, ref["ties"] >= 2) and (ref["gap_next"][lv] > 0.0).all()
    assert np.array_equal(ref["gap_next"][ref["ties"] == 1], ref["gap"][ref["ties"] == 1])
    assert c["hm"].nbytes <= 8 << 20 and c["hm"].dtype == np.float32


def test_the_references_take_a_few_seconds():
    """Measured here: 2 s for all of them, the 64-joint cases the longest at under 1 s each."""
    hc.golden()
    total = 0.0
    for name in NEW:
        c = hc.SWEEP[name]()
        t0 = time.perf_counter()
        ref = ho.triangulate(c["hm"], c["P"], c["flip"], c["plane"], c["X0"], c["image_shape"], c["half"], c["levels"], c["floor"])
        dt = time.perf_counter() - t0
        total += dt
        print(f"{name}: {dt * 1e3:.0f} ms for {int((ref['status'] != 0).sum())} searches of {c['levels']} levels")
    assert total < 10.0


def test_unequal_cells_everywhere_and_the_shapes_the_issue_names():
    shapes = {name: hc.sweep(name)["hm"].shape for name in NEW}
    assert [shapes[k][3:] for k in hc.FAMILIES["shapes"]] == [(4, 4), (5, 7), (16, 32), (96, 24), (1024, 1024)]
    for name in NEW:
        c = hc.sweep(name)
        rows, cols = ho.cell_size(c["image_shape"], *c["hm"].shape[3:])
        golden = "golden" in name or name.startswith("cut")
        assert rows != cols or golden
        if not golden:   # the exact cameras: 4 x 8 pixels, and a cell coordinate is the point's own coordinate to the bit
            assert (rows, cols) == (4.0, 8.0)
            X = np.random.default_rng(0).uniform(0.0, 1024.0, (64, 3))
            for v in range(len(c["P"])):
                row_px, col_px, w = ho.project(np.abs(c["P"][v]), X)
                r, col = ho.to_cells(row_px, col_px, False, (rows, cols), c["hm"].shape[4])
                assert np.array_equal(r, X[:, 1 + v % 2]) and np.array_equal(col, X[:, 0] + (v // 2) / 8.0) and (w == 1.0).all()
    assert ho.cell_size(hc.sweep("96x24 golden")["image_shape"], 96, 24) == (5.0, 40.0)      # unequal cells under perspective
    assert any(s[0] == 2 and s[2] == 3 and s[3:] != (64, 128) for s in shapes.values())       # frame, view and plane strides
    assert shapes["C 1024"][2:] == (1024, 4, 4) and sorted(hc.sweep("C 1024")["plane"].ravel().tolist()) == [0, 0, 1023, 1023]
    assert shapes["J 64, V 8"][1] == 8 and hc.sweep("J 64, V 8")["plane"].shape == (8, 64) and hc.sweep("J 1")["plane"].shape == (2, 1)
    assert shapes["1024x1024"] == (1, 2, 1, 1024, 1024)
    big = hc.sweep("1024x1024")["hm"][0, :, 0]
    assert (big[:, 1016:, 1016:].max(axis=(1, 2)) > 0.5).all()                              # a blob within 8 cells of the far corner, both views
    assert big[0].reshape(-1).argmax() > 1016 * 1024 + 1016 and hc.sweep("many")["hm"].shape == (4, 2, 64, 8, 8)
    assert 4 * hc.MANY_REPEAT * 64 == 70400 > 65535


def test_each_status_the_families_claim_occurs():
    status = {name: hc.sweep_reference(name)["status"] for name in NEW}
    assert (status["V 1"] == 0).all() and (hc.sweep_reference("V 1")["views"] == 1).all()
    assert status["floor"][0, 0] == 1 and status["floor"][0, 1] == 2 and status["floor"][0, 2] in (1, 3)
    for name in ("4x4", "5x7", "16x32", "96x24 golden", "1024x1024", "C 1024", "J 64, V 8", "J 1", "many", "budget 4096", "budget 4160"):
        assert (status[name] == 1).all(), name
    assert (status["budget behind"] == 3).all() and set(status["ties"].ravel().tolist()) == {1, 3}
    for name in hc.FAMILIES["cut"]:
        assert np.isin(status[name], (1, 3)).all(), name
    # the floor case's values: exactly the floor, one float32 step above and below, and nothing else under the blob's skirt
    c = hc.sweep("floor")
    f, up, down = c["values"]
    assert c["floor"] == 2.0 ** -10 == float(f) and down < f < up and float(up) - float(f) == 2.0 ** -33 and float(f) - float(down) == 2.0 ** -34
    for j, want in ((0, {f, up, down}), (1, {f, down}), (2, {f, up, down})):
        for v in range(2):
            cells = c["hm"][0, v, c["plane"][v, j]]
            assert set(cells[cells < 2.0 * f].tolist()) == {float(x) for x in want}, (j, v)
    assert all((c["hm"][0, v, c["plane"][v, 2]] == up).sum() == 1 for v in range(2)) and (c["hm"][0, :, c["plane"][0, 0]] > 0.5).any()


def test_the_tie_layouts_give_the_lower_index():
    c, ref = hc.sweep("ties"), hc.sweep_reference("ties")
    assert c["hm"].shape[3:] == (16, 32) and c["levels"] >= 2 and 2.0 * c["half"] / 8 == 1.0
    for k, (a, b) in enumerate(hc.TIE_PAIRS):
        pts, s = hc.level_points(c, ref, 0, k, 0)
        assert np.nonzero(s == s.max())[0].tolist() == [a, b] and a < b
        assert ref["choice"][0, k, 0] == a and ref["ties"][0, k, 0] == 2 and ref["gap"][0, k, 0] == 0.0 and ref["gap_next"][0, k, 0] > 0.1
        assert hc.tied_by_construction(c, ref, 0, k, 0)
        assert ref["ties"][0, k, 1] == 1 and ref["gap"][0, k, 1] > 1e-3            # the next level follows point a, and is plain
        assert np.abs(ref["points"][0, k] - pts[a]).max() <= c["half"] / 8 and np.abs(ref["points"][0, k] - pts[b]).max() > 0.5
    (a0, b0), (a1, b1), (a2, b2) = hc.TIE_PAIRS[:3]
    # the rest: at every step of the tree but the first, a pair whose higher index waits in the receiving lane
    assert [hc.tie_meeting(a, b) for a, b in hc.TIE_PAIRS[3:]] == [(1 << k, b) for k, (a, b) in enumerate(hc.TIE_PAIRS[3:])]
    assert len(hc.TIE_PAIRS) == 10 and hc.tie_meeting(a1, b1) == (4, a1) and hc.tie_meeting(a2, b2) == (4, a2)
    assert b0 == a0 + 256                               # a lane's own two points
    assert a1 < b1 and a1 % 256 > b1 % 256              # the lower index sits in the higher lane
    assert b2 - a2 == 4 and a2 // 8 == b2 // 8          # four steps apart along z
    # one view behind its camera: the eight points along z share every informed view's taps -- ties by construction at every level
    c, ref = hc.sweep("budget behind"), hc.sweep_reference("budget behind")
    assert (ref["ties"] == 8).all() and (ref["choice"] % 8 == 0).all() and hc.firm(c, ref).all()
    # a tie that two different computations happen to produce is not firm: the same patch in both views ties level 1 by commutativity
    same = dict(c=hc.sweep("ties"))
    hm = same["c"]["hm"].copy()
    hm[0, 1][hm[0, 1] > 0] = 0.0
    for k, pair in enumerate(hc.TIE_PAIRS):
        for i in pair:
            z, x = 8.0 + (i % 8 - 3.5), 12.0 + (i // 64 - 3.5)
            hm[0, 1, k, int(z) - 1:int(z) + 3, int(32 - x) - 1:int(32 - x) + 3] = hc.TIE_PATCH[0]
    c2 = dict(same["c"], hm=hm)
    ref2 = ho.triangulate(hm, c2["P"], c2["flip"], c2["plane"], c2["X0"], c2["image_shape"], c2["half"], c2["levels"], c2["floor"])
    assert (ref2["ties"][0, :, 1] == 2).all() and not hc.firm(c2, ref2).any()


def test_the_window_model_is_pinned():
    used = {name: hc.sweep_windows(name)[0] for name in hc.ROUTES}
    win = {name: hc.sweep_windows(name)[1] for name in hc.ROUTES}
    assert (used["budget 4096"] == 4096).all() and (used["budget 4160"] == 4160).all() and (used["budget behind"] == 2048).all()
    assert (win["budget 4096"] == [0, 31, 0, 63]).all() and (win["budget 4160"] == [0, 31, 0, 64]).all()
    assert (win["budget behind"][:, :, 0] == [0, 31, 0, 63]).all() and (win["budget behind"][:, :, 1] == [0, -1, 0, -1]).all()
    assert used["fly"].min() == 1265 and used["fly"].max() == 1936
    # special(8): one search passes the budget and takes the plane route beside staged neighbours
    s8, ref8 = used["special 8"], hc.sweep_reference("special 8")
    assert np.array_equal(s8 == 0, ref8["status"] == 0) and np.argwhere(s8 > 4096).tolist() == [[2, 2]] and s8[2, 2] == 4160
    assert ((s8 > 0) & (s8 <= 4096)).sum() == 6
    # cut w: the plane w = 0 of view 1 cuts the first joint's cube -- some corners before it, some behind: the whole plane
    c = hc.sweep("cut w")
    e = c["half"] * ho.REACH
    corners = c["X0"][0, 0] + e * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    w = ho.project(c["P"][1], corners)[2]
    assert abs(ho.project(c["P"][1], c["X0"][0, 0])[2] - 0.1) < 1e-9 and 0 < (w > 0).sum() < 8
    assert win["cut w"][0, 0, 1].tolist() == [0, 15, 0, 31] and used["cut w"].tolist() == [[692, 683, 683], [692, 683, 683]]
    whole = (win["cut w"][:, :, 1] == [0, 15, 0, 31]).all(axis=-1)
    none = (win["cut w"][:, :, 1] == [0, -1, 0, -1]).all(axis=-1)
    print(f"cut w: view 1 is cut in {int(whole.sum())} searches and wholly behind in {int(none.sum())} of {whole.size}; used {used['cut w'].tolist()}")
    # cut inf: corners with x > 0.8 project to an infinite column in view 1 while the start point is finite: the whole plane
    c = hc.sweep("cut inf")
    whole = (win["cut inf"][:, :, 1] == [0, 15, 0, 31]).all(axis=-1)
    finite0 = np.array([[np.isfinite(ho.project(c["P"][1], c["X0"][t, j])[1]) for j in range(6)] for t in range(2)])
    print(f"cut inf: whole plane in {int(whole.sum())} of {whole.size} searches, {int((whole & finite0).sum())} of them with a finite start; "
          f"used {used['cut inf'].tolist()}")
    assert whole.any() and not whole.all() and (whole & finite0).any() and np.isfinite(c["X0"]).all()
    assert used["cut inf"].max() == 692 and used["cut inf"].min() == 179
    for name in hc.ROUTES:   # every route case is staged at the default budget but for the two named above, and no searched joint has no window
        ref = hc.sweep_reference(name)
        assert np.array_equal(used[name] > 0, ref["status"] != 0), name
        assert (used[name] <= 4096).all() or name in ("special 8", "budget 4160"), name


@pytest.mark.parametrize("name", ["16x32", "5x7", "ties"])
def test_the_windows_of_the_exact_cameras_by_hand(name):
    """Cell coordinates are the point's own: view 0 sees rows y and columns x, view 1 rows z and columns W - x."""
    c = hc.sweep(name)
    used, win = hc.sweep_windows(name)
    H, W = c["hm"].shape[3:]
    e = 1.25 * c["half"]
    for t in range(c["X0"].shape[0]):
        for j in range(c["X0"].shape[1]):
            x, y, z = c["X0"][t, j]
            want = []
            for lo_r, hi_r, lo_c, hi_c in ((y - e, y + e, x - e, x + e), (z - e, z + e, W - (x + e), W - (x - e))):
                want.append([max(int(np.floor(lo_r)) - 1, 0), min(int(np.floor(hi_r)) + 2, H - 1), max(int(np.floor(lo_c)) - 1, 0),
                             min(int(np.floor(hi_c)) + 2, W - 1)])
            assert win[t, j].tolist() == want
            assert used[t, j] == sum((w[1] - w[0] + 1) * (w[3] - w[2] + 1) for w in want)


@pytest.mark.parametrize("name", ["fly", "special 8", "16x32", "96x24 golden", "ties", "cut w", "cut inf", "floor", "4x4"])
def test_every_tap_of_every_level_lies_in_its_window(name):
    """What the window is for: a search that stays in the cube it can reach reads staged cells only, so a window that is too small shows
    in nothing but `used`.  The model's windows hold every tap of every informed point of the oracle's own levels."""
    c, ref = hc.sweep(name), hc.sweep_reference(name)
    win = hc.sweep_windows(name)[1]
    H, W = c["hm"].shape[3:]
    cell = ho.cell_size(c["image_shape"], H, W)
    reads = 0
    for t, j, level in zip(*np.nonzero(ref["choice"] >= 0)):
        pts = hc.level_points(c, ref, t, j, level)[0]
        for v in range(len(c["P"])):
            if c["plane"][v, j] < 0:
                continue
            row_px, col_px, w = ho.project(c["P"][v], pts)
            r, col = ho.to_cells(row_px, col_px, bool(c["flip"][v]), cell, W)
            with np.errstate(invalid="ignore"):
                ok = (w > 0.0) & (r >= 0.0) & (r <= H - 1.0) & (col >= 0.0) & (col <= W - 1.0)
            if not ok.any():
                continue
            r0, r1, c0, c1 = win[t, j, v]
            assert np.clip(np.floor(r[ok]) - 1, 0, H - 1).min() >= r0 and np.clip(np.floor(r[ok]) + 2, 0, H - 1).max() <= r1
            assert np.clip(np.floor(col[ok]) - 1, 0, W - 1).min() >= c0 and np.clip(np.floor(col[ok]) + 2, 0, W - 1).max() <= c1
            reads += int(ok.sum())
    assert reads > 0
