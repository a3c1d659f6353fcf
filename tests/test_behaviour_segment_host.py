"""CPU tests of the behaviour map's segmentation: the float64 model of tests/behaviour_segment_oracle.py against
properties that need no device, the bar of the density against the separable form the device computes, and the refusals of the
host side."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import behaviour_segment_oracle as bo  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ density
def test_density_integrates_to_one_within_the_tail_mass():
    """Every frame's Gaussian lies at least 3 sigma inside the grid on all four sides, so at most 4 Q(3) of it is cut off; the
    midpoint rule on cells of h = 38 sigma / G adds nothing visible at G >= 64 (its error falls like exp(-2 pi^2 sigma^2 / h^2))."""
    tail = 4.0 * bo.gaussian_tail(3.0)
    for M, T, G in ((257, 260, 64), (1031, 1040, 96)):
        Y = bo.density_case(M, T)
        origin, sigma = bo.grid(Y, G)
        rho, _ = bo.density(Y, origin, sigma, G)
        mass = float(rho.sum() * origin[2] ** 2)
        print(f"M = {M}, G = {G}: sum rho h^2 = {mass:.9f}, 1 - mass = {1 - mass:.3g}, the tail bound 4 Q(3) = {tail:.3g}")
        assert 1.0 - tail - 1e-9 <= mass <= 1.0 + 1e-9
        assert origin[2] * G == pytest.approx(2 * (16 + 3) * sigma)   # L = ext / 2 + 3 sigma with sigma = ext / 32


@pytest.mark.parametrize("M,T,G", bo.DENSITY_CASES)
def test_separable_form_stays_inside_the_density_bar(M, T, G):
    """What the bar rests on: the device's form, two exponentials and a matrix product in slices, in numpy."""
    Y = bo.density_case(M, T)
    assert int(bo.valid_rows(Y).sum()) == M and len(Y) == T
    for sigma in (None if M > 1 else 1.0, 0.02):   # one frame has no extent and so no default sigma
        origin, sigma = bo.grid(Y, G, sigma)
        rho, A = bo.density(Y, origin, sigma, G)
        sep = bo.density_separable(Y, origin, sigma, G)
        bar = bo.density_tolerance(rho, A, M)
        frac = float((np.abs(sep - rho) / bar).max())
        print(f"M = {M}, G = {G}, sigma = {sigma:.3g}: the separable form is up to {frac:.3g} of the bar from the oracle; A up to {A.max():.3g}, "
              f"{int((rho == 0).sum())} cells exactly 0")
        assert frac <= 1.0
        assert np.all(np.abs(sep[rho == 0]) < 2.3e-308)   # 0 or denormal where the oracle is exactly 0
    if M > 1:
        assert (rho == 0).any()   # the small sigma underflows in the far cells


def test_invalid_rows_contribute_nothing():
    Y = bo.density_case(257, 260)
    origin, sigma = bo.grid(Y, 16)
    rho, _ = bo.density(Y, origin, sigma, 16)
    clean = Y[bo.valid_rows(Y)]
    assert np.array_equal(bo.density(clean, origin, sigma, 16)[0], rho) and np.isfinite(rho).all()
    assert bo.grid(clean, 16) == (origin, sigma)


# ------------------------------------------------------------------------------------------------------------------ watershed
def test_watershed_on_built_fields():
    f = bo.built_fields()
    res = {name: bo.watershed(*args) for name, args in f.items()}
    regions, R, roots, _ = res["one peak"]
    assert R == 1 and list(roots) == [5 * 12 + 7] and np.all(regions == 1)
    regions, R, roots, _ = res["two equal peaks"]
    assert R == 2 and list(roots) == [3 * 12 + 3, 8 * 12 + 8] and regions[3, 3] == 1 and regions[8, 8] == 2
    assert (regions == 1).sum() + (regions == 2).sum() == 144 and abs(int((regions == 1).sum()) - 72) <= 12   # ties on the diagonal go to one side
    regions, R, roots, longest = res["all equal"]
    assert R == 1 and list(roots) == [0] and np.all(regions == 1) and longest == 6   # every cell climbs towards index 0
    regions, R, roots, _ = res["all zero"]
    assert R == 0 and len(roots) == 0 and np.all(regions == 0)   # a root needs rho > 0, also with min_peak = 0
    regions, R, roots, _ = res["plateau touching a higher cell"]
    # the plateau's cell (5, 5) touches the higher cell and climbs to it; the rest of the plateau climbs to the plateau's
    # smallest index, (2, 2), which no higher cell touches: two regions
    assert R == 2 and list(roots) == [2 * 9 + 2, 6 * 9 + 6] and regions[5, 5] == 2 and regions[2, 2] == 1 and regions[4, 4] == 1
    regions, R, roots, _ = res["zeros round a bump, min_peak 0"]
    assert R == 1 and list(roots) == [6 * 12 + 6] and regions[6, 6] == 1
    zero_plateau_roots = regions[0, 0]   # the far zeros climb towards index 0, whose density is 0: never a region
    assert zero_plateau_roots == 0 and (regions == 0).any() and (regions == 1).sum() >= 25
    assert np.array_equal(res["zeros round a bump, min_peak 0.5"][0], regions)
    assert res["a minor peak kept"][1] == 2 and res["a minor peak dropped"][1] == 1
    dropped = res["a minor peak dropped"][0]
    assert dropped[9, 9] == 0 and dropped[3, 3] == 1 and np.array_equal(dropped == 1, res["a minor peak kept"][0] == 1)
    regions, R, roots, longest = res["spiral ridge"]
    G = f["spiral ridge"][0].shape[0]
    assert longest > 2 ** 7 > G and int(np.ceil(np.log2(G * G))) == 9   # 8 rounds of doubling are needed, log2 G rounds would not do
    assert R == 1 and np.all(regions == 1)
    assert res["two by two"][1] == 1 and list(res["two by two"][2]) == [0]   # min_peak = 1: the maximum itself is kept


def test_pointers_rise_strictly_so_there_are_no_cycles():
    rng = np.random.default_rng(5)
    rho = rng.integers(0, 4, size=(15, 15)).astype(np.float64)   # many ties
    ptr = bo.ascent(rho)
    flat = rho.ravel()
    for i, p in enumerate(ptr):
        assert p == i or bo._above(flat[p], p, flat[i], i)
    regions, R, roots, _ = bo.watershed(rho, 0.0)
    assert np.all(np.diff(roots) > 0) and [regions.ravel()[c] for c in roots] == list(range(1, R + 1))


# ------------------------------------------------------------------------------------------------------------------ labels, ethogram
def test_labels_on_cell_edges_and_the_outer_border():
    G, origin = 4, (-2.0, 10.0, 0.5)   # columns [-2, -1.5), ... [-0.5, 0]; rows [10, 10.5), ... [11.5, 12]
    regions = np.arange(1, 17, dtype=np.int32).reshape(4, 4)
    Y = np.array([[-2.0, 10.0], [-1.5, 10.0], [-1.5000000000000002, 10.5], [0.0, 12.0], [5.0, 99.0], [-7.0, 9.999], [-0.5, 11.5],
                  [np.nan, 10.0], [-1.0, np.inf], [-1e308, 1e308]])
    want = [1, 2, 5, 16, 16, 1, 16, -1, -1, 13]
    assert list(bo.labels(Y, regions, origin)) == want


def test_bouts_of_a_hand_written_row():
    lab = np.array([-1, -1, 0, 0, 0, 2, 2, 1, 2, -1, 1, 1, 0], dtype=np.int32)
    bouts, occupancy, transitions = bo.ethogram(lab, 2)
    assert bouts.tolist() == [[-1, 0, 2], [0, 2, 3], [2, 5, 2], [1, 7, 1], [2, 8, 1], [-1, 9, 1], [1, 10, 2], [0, 12, 1]]
    assert occupancy.tolist() == [4, 3, 3]
    assert transitions.tolist() == [[0, 0, 1], [1, 0, 1], [0, 1, 0]]   # 0 -> 2, 2 -> 1, 1 -> 2, 1 -> 0; nothing across the -1
    assert bouts.dtype == occupancy.dtype == transitions.dtype == np.int64


@pytest.mark.parametrize("T", bo.SCAN_SIZES)
@pytest.mark.parametrize("kind", ["random", "single", "alternating"])
def test_ethogram_sums(T, kind):
    lab = bo.label_row(T, kind)
    bouts, occupancy, transitions = bo.ethogram(lab, 5)
    assert bouts[:, 2].sum() == T and np.all(bouts[:, 2] >= 1) and np.all(bouts[1:, 0] != bouts[:-1, 0])
    assert np.array_equal(bouts[:, 1], np.concatenate(([0], np.cumsum(bouts[:, 2])[:-1])))
    assert np.array_equal(occupancy, np.bincount(lab[lab >= 0], minlength=6))
    pairs = [(a, b) for a, b in zip(lab[:-1], lab[1:]) if a >= 0 and b >= 0 and a != b]
    assert transitions.sum() == len(pairs) and not np.diag(transitions).any()
    if kind == "single":
        assert bouts.tolist() == [[2, 0, T]]
    if kind == "alternating":
        assert len(bouts) == T


# ------------------------------------------------------------------------------------------------------------------ the planted case
@pytest.mark.parametrize("G", bo.PLANTED["grids"])
def test_planted_case_gives_three_pure_regions(G):
    Y, behaviour = bo.planted_case()
    for min_peak in (bo.PLANTED["keep_three"], bo.PLANTED["keep_four"]):
        s = bo.segment(Y, G, bo.PLANTED["sigma"], min_peak)
        bo.check_planted(s["labels"], s["R"], behaviour, min_peak)
        assert s["bouts"][:, 2].sum() == len(Y) and s["occupancy"].sum() == len(Y) - 2
        near = np.abs(s["region_peaks"][:3, None, :] - bo.PLANTED_CENTRES[None]).max(axis=2).min(axis=1)
        assert np.all(near <= 1.0 + s["origin"][2])   # every kept peak within a cell and a deviation of a planted centre


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_model_refusals():
    with pytest.raises(ValueError, match="no valid frame"):
        bo.grid(np.full((3, 2), np.nan), 16)
    with pytest.raises(ValueError, match="no extent"):
        bo.grid(np.ones((3, 2)), 16)
    assert bo.grid(np.ones((3, 2)), 16, 0.5) == ((1.0 - 1.5, 1.0 - 1.5, 3.0 / 16), 0.5)


def test_host_side_refusals():
    """ops refuses on the host, before any device is needed."""
    import torch

    from deepfly3d_amd import config, ops

    assert (config.BEHAVIOUR_GRID, config.BEHAVIOUR_DENSITY_SIGMA_FRACTION, config.BEHAVIOUR_MIN_PEAK) == (bo.GRID, bo.SIGMA_FRACTION, bo.MIN_PEAK)
    assert config.BEHAVIOUR_GRID_RANGE == bo.GRID_RANGE
    for bad in (1, 1025, 2.5, True, "64"):
        with pytest.raises(ValueError, match=r"grid must be an integer in \[2, 1024\]"):
            ops.density_grid((0, 0), (1, 1), bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma must be finite and > 0"):
            ops.density_grid((0, 0), (1, 1), 16, bad)
    with pytest.raises(ValueError, match="lies on one point.*give sigma"):
        ops.density_grid((2, 3), (2, 3), 16)
    assert ops.density_grid((2, 3), (2, 3), 16, 0.5) == ((0.5, 1.5, 3.0 / 16), 0.5)
    Y = bo.density_case(257, 260)
    v = Y[bo.valid_rows(Y)]
    for G, sigma in ((16, None), (33, 0.3), (256, None)):   # the host's grid is the oracle's, to the bit
        assert ops.density_grid(v.min(axis=0), v.max(axis=0), G, sigma) == bo.grid(Y, G, sigma)
    with pytest.raises(ValueError, match=r"Y must be a torch.float64 CUDA tensor of shape \[T, 2\]"):
        ops.map_density(torch.zeros((4, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="Y must be"):
        ops.segment_map(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="rho must be"):
        ops.watershed(torch.zeros((4, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="labels must be"):
        ops.ethogram(torch.zeros((4,), dtype=torch.int32), 2)
    assert ops.BehaviourSegmentsResult._fields == ("density", "origin", "sigma", "regions", "region_peaks", "labels", "bouts", "occupancy",
                                                   "transitions")


def test_command_line_refusals(capsys):
    from deepfly3d_amd import cli

    for argv, message in ((["x", "--behaviour-segments"], "--behaviour-segments segments the map of --behaviour-map: it needs --behaviour-map"),
                          (["x", "--behaviour-map", "--behaviour-sigma", "2"], "--behaviour-sigma .* needs --behaviour-segments"),
                          (["x", "--behaviour-map", "--behaviour-grid", "64"], "--behaviour-grid .* needs --behaviour-segments"),
                          (["x", "--behaviour-map", "--behaviour-segments", "--behaviour-sigma", "0"], "--behaviour-sigma must be finite and > 0"),
                          (["x", "--behaviour-map", "--behaviour-segments", "--behaviour-grid", "1"], r"--behaviour-grid must be in \[2, 1024\]")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err)
    parse = cli.parse_cli_args
    args = parse(["x", "--behaviour-map", "--behaviour-segments", "--behaviour-sigma", "2.5", "--behaviour-grid", "64"])
    assert args.behaviour_segments and args.behaviour_sigma == 2.5 and args.behaviour_grid == 64
    args = parse(["x", "--behaviour-map"])
    assert not args.behaviour_segments and args.behaviour_sigma is None and args.behaviour_grid is None
