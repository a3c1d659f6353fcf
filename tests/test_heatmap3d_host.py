"""CPU tests of the heat-map triangulation's model (tests/heatmap3d_oracle.py) against itself, and of the host side of
deepfly3d_amd/heatmap3d.py: the pixel <-> cell rule, the sampler, planted blobs, the statuses, the view table and the refusals."""
import numpy as np
import pytest

import heatmap3d_cases as hc
import heatmap3d_oracle as ho

STEP = 2.0 * hc.HALF / 8 / 4 ** (hc.LEVELS - 1)   # the last level's step: 0.0015625 mm at the defaults


def test_the_defaults_are_the_cases():
    from deepfly3d_amd import config

    assert (config.HEATMAP3D_HALF, config.HEATMAP3D_LEVELS, config.HEATMAP3D_FLOOR, config.HEATMAP3D_GRID) == (hc.HALF, hc.LEVELS, hc.FLOOR, ho.GRID)
    assert STEP == 0.0015625


@pytest.mark.parametrize("flipped", [False, True])
def test_a_single_cell_is_sampled_where_the_relayout_puts_it(flipped):
    """The arg-max of a plane that is one cell at (r, c) is (r / H, c / W) in float32; relayout_kernel un-flips the column (col -> 1 - col,
    float64) and df3d_triangulate_scaled multiplies by the image shape.  Sampling the plane at that pixel returns the cell's l exactly."""
    H, W = hc.H, hc.W
    cols, rows = hc.IMAGE_SHAPE
    cell = ho.cell_size(hc.IMAGE_SHAPE, H, W)
    lf = float(np.log(hc.FLOOR))
    for r, c, h in ((0, 0, 0.5), (17, 93, 0.73), (63, 127, 1.0), (5, 1, 0.0123), (40, 64, 0.999)):
        plane = np.zeros((H, W), dtype=np.float32)
        plane[r, c] = h
        L = ho.cell_logs(plane, hc.FLOOR, lf)
        row, col = float(np.float32(r) / np.float32(H)), float(np.float32(c) / np.float32(W))     # heatmap_argmax's point
        if flipped:
            col = 1.0 - col                                                                       # relayout_kernel
        row_px, col_px = row * rows, col * cols                                                   # df3d_triangulate_scaled
        rr, cc = ho.to_cells(np.array(row_px), np.array(col_px), flipped, cell, W)
        assert (float(rr), float(cc)) == (float(r), float(c))
        got = ho.sample(L, rr, cc, lf)
        assert float(got) == float(np.log(np.float64(np.float32(h)))) == L[r, c]


def test_catmull_rom_reproduces_a_quadratic():
    rng = np.random.default_rng(3)
    H, W = 24, 40
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    worst = 0.0
    for _ in range(20):
        a = rng.normal(0.0, 0.05, 6)

        def q(r, c):
            return a[0] * r * r + a[1] * r * c + a[2] * c * c + a[3] * r + a[4] * c + a[5] - 7.0

        r, c = rng.uniform(1.0, H - 2.0, 200), rng.uniform(1.0, W - 2.0, 200)   # away from the clamped border, where the taps repeat
        worst = max(worst, float(np.abs(ho.sample(q(rr, cc), r, c) - q(r, c)).max()))
    print(f"Catmull-Rom on quadratics: worst |sample - value| {worst:.2e}")
    assert worst <= 1e-12
    f = rng.uniform(0.0, 1.0, 1000)
    assert np.abs(np.sum(ho.weights(f), axis=0) - 1.0).max() <= 4 * np.finfo(np.float64).eps


def _errors(case, ref):
    return np.linalg.norm(ref["points"] - case["planted"], axis=-1)


@pytest.mark.parametrize("second", [False, True])
def test_planted_blobs_at_three_views(second):
    """Four golden frames, the 30 joints three cameras see, the defaults.  rms <= one final step; every point within sqrt(3) / 2 of a
    step of the planted one (half a step per axis from the score's maximum, which for Gaussian blobs is the planted point; the float32
    rounding of the maps moves l by 6e-8 against a curvature of 1 per cell^2, 1e-8 mm: 1e-6 mm is allowed for it).  With a 1.3 x
    stronger second blob 6 cells away in one view the same bars hold, and the arg-max of those maps is off by more than 0.1 mm."""
    case, ref = hc.fly(4, 0.0, second, 3), hc.reference("fly", 4, 0.0, second, 3)
    assert case["plane"].shape == (6, 30) and ((case["plane"] >= 0).sum(axis=0) == 3).all()
    e = _errors(case, ref)
    rms = float(np.sqrt((e ** 2).mean()))
    print(f"second blob {second}: rms {rms:.6f} mm = {rms / STEP:.2f} step, max {e.max() / STEP:.2f} step, smallest gap {ref['gap'].min():.2e}")
    assert (ref["status"] == 1).all() and (ref["views"][:, :15] == 0b000111).all() and (ref["views"][:, 15:] == 0b111000).all()
    assert rms <= STEP
    assert e.max() <= np.sqrt(3.0) / 2.0 * STEP + 1e-6
    assert np.allclose(ref["shift"], np.linalg.norm(ref["points"] - case["X0"], axis=-1), rtol=0, atol=1e-15)
    assert ref["counts"].tolist() == [[0, 4, 0, 0]] * 30
    if second:
        a = ho.argmax_dlt(case["hm"], case["P"], case["flip"], case["plane"], hc.IMAGE_SHAPE)
        rms_argmax = float(np.sqrt((np.linalg.norm(a - case["planted"], axis=-1) ** 2).mean()))
        print(f"arg-max + DLT on the same maps: rms {rms_argmax:.3f} mm")
        assert rms_argmax > 0.1


def test_two_views_cannot_tell_two_blobs_apart():
    """The stated limit: with two views the stronger blob of a view wins wherever its ray passes the other view's blob."""
    case, ref = hc.fly(2, 0.0, True, 2), hc.reference("fly", 2, 0.0, True, 2)
    e = _errors(case, ref)[:, (case["plane"] >= 0).sum(axis=0) == 2]
    print(f"two views, second blob: rms {np.sqrt((e ** 2).mean()):.3f} mm")
    assert (e > 0.1).any()


@pytest.mark.parametrize("V", [2, 3, 8])
def test_statuses_on_constructed_inputs(V):
    case, ref = hc.special(V), hc.reference("special", V)
    assert ref["status"].tolist() == [[1, 1, 3, 0], [0, 0, 1, 0], [2, 1, 1, 0]]
    assert ref["counts"].tolist() == [[1, 1, 1, 0], [1, 2, 0, 0], [0, 2, 0, 1], [3, 0, 0, 0]]
    keeps = ref["status"] != 1
    keeps[0, 2] = False
    assert ref["points"][keeps].tobytes() == case["X0"][keeps].tobytes()            # the bits of X0, its NaN included
    assert np.isnan(ref["score"][ref["status"] == 0]).all() and not ref["shift"][keeps].any()
    lf = float(np.log(hc.FLOOR))
    assert ref["score"][2, 0] == sum([lf] * V) and (ref["choice"][2, 0] == -1).all() and (ref["choice"][ref["status"] == 0] == -1).all()
    assert (ref["views"][:, :3] == (1 << V) - 1).all() and (ref["views"][:, 3] == 1).all()
    first = ref["choice"][0, 2, 0]
    assert 7 in (first // 64, first // 8 % 8, first % 8) or 0 in (first // 64, first // 8 % 8, first % 8)
    assert _errors(case, ref)[0, 2] < 0.01                                          # the search followed the blob out of the cube
    assert (ref["gap"][ref["status"] % 2 == 1] > hc.GAP).all()
    # the non-finite and negative cells of frame 2, joint 1 are floor cells: the point stays at the blob
    assert _errors(case, ref)[2, 1] < 0.05


def test_view_table_follows_the_relayout_rule(golden_dir):
    """plane[v, j] is the network joint that df3d::relayout_source (csrc/geometry_dev.h) reads for the camera's position in the ordering,
    restated here; flip is its `left`."""
    import json

    from deepfly3d_amd.heatmap3d import view_table

    def source(pos, j):
        src = -1
        if pos < 3 and j < 19:
            src = j
        if 4 <= pos < 7 and j >= 19:
            src = j - 19
        if (pos == 2 and j >= 15) or (pos == 4 and j >= 19 + 15):
            src = -1
        return src, 4 <= pos < 7

    clc = [int(c) for c in np.load(f"{golden_dir}/relayout_clc.npz")["camera_ordering"]]
    assert sorted(clc) == list(range(7)) and clc != list(range(7))
    for order in (list(range(7)), list(range(7))[::-1], clc):
        cameras, flip, plane = view_table(order)
        assert cameras.tolist() == sorted(order[p] for p in (0, 1, 2, 4, 5, 6)) and plane.shape == (6, 38) and plane.dtype == np.int32
        for v, cam in enumerate(cameras):
            pos = order.index(cam)
            assert [source(pos, j)[0] for j in range(38)] == plane[v].tolist() and bool(flip[v]) == source(pos, 0)[1]
    assert json.dumps(view_table()[0].tolist()) == json.dumps(view_table(list(range(7)))[0].tolist())


def test_parameter_refusals():
    from deepfly3d_amd import config
    from deepfly3d_amd.heatmap3d import heatmap3d_params

    assert heatmap3d_params() == (config.HEATMAP3D_HALF, config.HEATMAP3D_LEVELS, config.HEATMAP3D_FLOOR)
    assert heatmap3d_params(1, 6, 0.5) == (1.0, 6, 0.5) and heatmap3d_params(np.float32(0.25), np.int64(1), 1e-30) == (0.25, 1, 1e-30)
    for bad in (0.0, -1.0, np.inf, np.nan, "1", True, None.__class__):
        with pytest.raises(ValueError, match="half must be a finite number > 0"):
            heatmap3d_params(half=bad)
    for bad in (0, 7, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"levels must be an integer in \[1, 6\]"):
            heatmap3d_params(levels=bad)
    for bad in (0.0, 1.0, -0.1, 2.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="floor must be a number with 0 < floor < 1"):
            heatmap3d_params(floor=bad)
    for bad in ("1e-3", True):
        with pytest.raises(ValueError, match="floor must be a number"):
            heatmap3d_params(floor=bad)


def test_cli_flags_and_the_save_signature(capsys):
    import inspect

    from deepfly3d_amd import cli
    from deepfly3d_amd.core import Core

    a = cli.parse_cli_args(["/data/x", "--heatmap-triangulation", "--heatmap-half", "0.2", "--heatmap-levels", "3", "--heatmap-floor", "1e-4",
                            "--skip-pose-estimation"])
    assert (a.heatmap_triangulation, a.heatmap_half, a.heatmap_levels, a.heatmap_floor) == (True, 0.2, 3, 1e-4)
    a = cli.parse_cli_args(["/data/x"])
    assert (a.heatmap_triangulation, a.heatmap_half, a.heatmap_levels, a.heatmap_floor) == (False, None, None, None)
    for argv, text in ((["--heatmap-half", "0.2"], "--heatmap-half sets a parameter of --heatmap-triangulation"),
                       (["--heatmap-levels", "2"], "--heatmap-levels sets a parameter of --heatmap-triangulation"),
                       (["--heatmap-floor", "0.01"], "--heatmap-floor sets a parameter of --heatmap-triangulation"),
                       (["--heatmap-triangulation", "--heatmap-levels", "7"], "levels must be an integer in [1, 6]"),
                       (["--heatmap-triangulation", "--heatmap-half", "-1"], "half must be a finite number > 0"),
                       (["--heatmap-triangulation", "--heatmap-floor", "1"], "floor must be a number with 0 < floor < 1")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(["/data/x", *argv])
        assert text in capsys.readouterr().err
    save = inspect.signature(Core.save).parameters
    assert [save[n].default for n in ("heatmap_triangulation", "heatmap_half", "heatmap_levels", "heatmap_floor")] == [False, None, None, None]
    assert list(inspect.signature(Core.heatmap_triangulation).parameters) == ["self", "half", "levels", "floor"]
    assert Core._HEATMAP3D_KEYS == ("points3d_heatmap", "heatmap3d_status", "heatmap3d_score", "heatmap3d_views", "heatmap3d_shift",
                                    "heatmap3d_counts", "heatmap3d_params")
