"""CPU tests of the sub-pixel localisation of heat-map peaks: the float64 oracle's accuracy on Gaussian planes,
the branch every special case takes, the argument validation of the new C entries and the CLI flag (no device is touched)."""
import ctypes

import numpy as np
import pytest

import subpixel_oracle as so

H, W = 64, 128


def _gaussian_errors(sigma, noise=0.0, n=2000, seed=0, margin=3.0):
    """Distances (cells) of the arg-max cell and of the refined point from the true centre, for n centres drawn uniformly at least
    `margin` cells from the border."""
    rng = np.random.default_rng(seed)
    cr = rng.uniform(margin, H - 1 - margin, size=n)
    cc = rng.uniform(margin, W - 1 - margin, size=n)
    plain, refined = np.empty(n), np.empty(n)
    for i in range(n):
        plane = so.gaussian_plane(cr[i], cc[i], sigma, (H, W))
        if noise:
            plane = (plane + rng.normal(0.0, noise, size=plane.shape)).astype(np.float32)
        r, c = np.unravel_index(int(plane.argmax()), plane.shape)
        dy, dx, _ = so.refine_cell(plane, int(r), int(c))
        plain[i] = np.hypot(r - cr[i], c - cc[i])
        refined[i] = np.hypot(r + dy - cr[i], c + dx - cc[i])
    return plain, refined


@pytest.mark.parametrize("sigma", [1.0, 1.5, 2.0])
def test_oracle_recovers_gaussian_centres(sigma):
    """The bounds are those of the table in DESIGN.md section 12 (mean 0.036 / 0.015 / 0.008, maximum 0.055 / 0.043 / 0.031 cells
    refined against 0.38 mean for the cell), computed with this oracle."""
    plain, refined = _gaussian_errors(sigma)
    print(f"sigma {sigma}: arg-max mean {plain.mean():.4f} max {plain.max():.4f}; refined mean {refined.mean():.4f} max {refined.max():.4f}")
    assert refined.mean() <= 0.05 and refined.max() <= 0.1
    assert plain.mean() >= 0.3


def _plane(values3x3, r=10, c=20, base=0.0):
    p = np.full((H, W), base, np.float32)
    p[r - 1 : r + 2, c - 1 : c + 2] = np.asarray(values3x3, np.float32)
    return p


def test_border_cells_keep_the_cell():
    rng = np.random.default_rng(1)
    plane = rng.normal(size=(H, W)).astype(np.float32)
    for r, c in [(0, 5), (H - 1, 5), (7, 0), (7, W - 1), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        assert so.refine_cell(plane, r, c) == (0.0, 0.0, so.BORDER)
        row, col = so.refine_point(plane, r, c)
        assert row == np.float32(r) / np.float32(H) and col == np.float32(c) / np.float32(W)
    # the "unseen" marker of the 38-joint layout is a coordinate that is exactly 0: no refined coordinate of an interior cell is 0 or 1
    for r, c in [(1, 1), (H - 2, W - 2)]:
        row, col = so.refine_point(plane, r, c)
        assert 0.0 < row < 1.0 and 0.0 < col < 1.0


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("where", [(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)])
def test_nonfinite_neighbourhood_keeps_the_cell(bad, where):
    n = np.array([[0.1, 0.3, 0.1], [0.4, 1.0, 0.2], [0.1, 0.5, 0.1]], np.float32)
    n[where] = bad
    assert so.refine_cell(_plane(n), 10, 20) == (0.0, 0.0, so.NONFINITE)


def test_flat_plane_has_no_offset():
    plane = np.full((H, W), 0.25, np.float32)
    assert so.refine_cell(plane, 10, 20) == (0.0, 0.0, so.PER_AXIS)   # no axis has a negative second difference
    pts, conf = so.heatmap_argmax_subpixel(plane[None, None])
    assert np.array_equal(pts, np.zeros((1, 1, 2), np.float32)) and conf[0, 0] == np.float32(0.25)   # cell 0: a border cell


def test_proper_maximum_takes_the_newton_step():
    n = [[0.50, 0.80, 0.60], [0.70, 1.00, 0.90], [0.40, 0.75, 0.65]]
    dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
    assert branch == so.NEWTON and abs(dy) <= 0.5 and abs(dx) <= 0.5
    assert dx > 0 and dy < 0   # towards the larger neighbours: right (0.9 > 0.7) and up (0.8 > 0.75)
    # without a cross term the Newton step is the two 1-D steps: -g / h = 0.1 / 0.8 along x, -0.1 / 1.0 along y
    n = [[0.10, 0.60, 0.10], [0.50, 1.00, 0.70], [0.10, 0.40, 0.10]]
    dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
    assert branch == so.NEWTON and abs(dx - 0.125) < 1e-6 and abs(dy + 0.1) < 1e-6


def test_saddle_treats_each_axis_alone():
    # both second differences negative but a cross term so large that det <= 0: the cell is the maximum of its 3 x 3 neighbourhood
    n = [[0.99, 0.90, 0.00], [0.92, 1.00, 0.90], [0.00, 0.94, 0.99]]
    p = _plane(n)
    v = np.asarray(n, np.float64)
    hxx, hyy = v[1, 2] - 2 * v[1, 1] + v[1, 0], v[2, 1] - 2 * v[1, 1] + v[0, 1]
    hxy = 0.25 * (v[2, 2] - v[2, 0] - v[0, 2] + v[0, 0])
    assert hxx < 0 and hyy < 0 and hxx * hyy - hxy * hxy < 0
    dy, dx, branch = so.refine_cell(p, 10, 20)
    assert branch == so.PER_AXIS
    assert abs(dx - (-(0.5 * (v[1, 2] - v[1, 0])) / hxx)) < 1e-6 and abs(dy - (-(0.5 * (v[2, 1] - v[0, 1])) / hyy)) < 1e-6
    assert abs(dx) <= 0.5 and abs(dy) <= 0.5


def test_step_outside_the_half_cell_is_clamped_per_axis():
    # a proper maximum of the quadratic (hxx = hyy = -0.9, hxy = 0.4, det = 0.65) whose Newton step, 0.7 on both axes, leaves the half
    # cell: each axis then takes its own 1-D step 0.35 / 0.9
    n = [[0.60, 0.20, 0.00], [0.20, 1.00, 0.90], [0.00, 0.90, 1.00]]
    dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
    assert branch == so.PER_AXIS and abs(dx - 0.35 / 0.9) < 1e-6 and abs(dy - 0.35 / 0.9) < 1e-6
    # the right neighbour equals the cell (the first-index tie-break made this one the arg-max): a step of exactly half a cell is taken
    n = [[0.10, 0.50, 0.10], [0.20, 1.00, 1.00], [0.10, 0.50, 0.10]]
    dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
    assert branch == so.NEWTON and dx == 0.5 and dy == 0.0
    # a cell that is no maximum along x (the rule is defined for any cell): -g / h = 1.5, clamped
    n = [[0.10, 0.50, 0.10], [0.00, 1.00, 1.50], [0.10, 0.50, 0.10]]
    dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
    assert branch == so.PER_AXIS and dx == 0.5 and dy == 0.0
    # an axis without a maximum (second difference >= 0) does not move
    n = [[0.10, 1.00, 0.10], [0.20, 1.00, 0.30], [0.10, 1.00, 0.10]]
    dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
    assert branch == so.PER_AXIS and dy == 0.0 and 0.0 < dx <= 0.5


def test_every_offset_lies_in_the_half_cell():
    rng = np.random.default_rng(2)
    branches = set()
    for trial in range(4000):
        n = rng.normal(size=(3, 3)).astype(np.float32)
        if trial % 2:
            n[1, 1] = n.max() + np.float32(rng.uniform(0, 0.5))   # a local maximum, as the kernels pass
        dy, dx, branch = so.refine_cell(_plane(n), 10, 20)
        branches.add(branch)
        assert -0.5 <= dy <= 0.5 and -0.5 <= dx <= 0.5
    assert branches == {so.NEWTON, so.PER_AXIS}


def test_oracle_argmax_cell_is_the_plain_oracles():
    from oracle import geometry as og

    rng = np.random.default_rng(3)
    hm = rng.integers(0, 6, size=(3, 5, 8, 16)).astype(np.float32)   # many ties
    rows, cols = so.argmax_cells(hm)
    am, conf = og.heatmap_argmax(hm)
    assert np.array_equal(rows.astype(np.float32) / np.float32(8), am[..., 0]) and np.array_equal(cols.astype(np.float32) / np.float32(16), am[..., 1])
    pts, c2 = so.heatmap_argmax_subpixel(hm)
    assert np.array_equal(c2, conf) and np.all(np.abs(pts - am) <= np.array([0.5 / 8, 0.5 / 16], np.float32))


def test_new_entries_validate_arguments_without_gpu(native_lib):
    p16 = ctypes.c_void_p(4096)
    lib = native_lib
    am = lib.df3d_heatmap_argmax_subpixel
    assert am(None, 1, 19, 3, 5, None, None, None, None) == -1 and b"multiple of 4" in lib.df3d_last_error()
    assert am(p16, 1, 0, 64, 128, p16, p16, None, None) == -1 and b"bad shape" in lib.df3d_last_error()
    assert am(p16, 1, 19, 48, 128, p16, p16, None, None) == -1 and b"powers of two" in lib.df3d_last_error()
    assert am(ctypes.c_void_p(4100), 1, 19, 64, 128, p16, p16, None, None) == -1 and b"16-byte" in lib.df3d_last_error()
    assert am(None, 1, 19, 64, 128, None, None, None, None) == -1 and b"null" in lib.df3d_last_error()
    assert am(None, 0, 19, 64, 128, None, None, None, None) == 0   # nothing to do
    pk = lib.df3d_heatmap_peaks_subpixel
    assert pk(p16, 1, 19, 64, 128, 17, p16, p16, p16, None) == -1 and b"k must be" in lib.df3d_last_error()
    assert pk(p16, 1, 19, 48, 128, 4, p16, p16, p16, None) == -1 and b"powers of two" in lib.df3d_last_error()
    assert pk(p16, 1, 19, 128, 128, 4, p16, p16, p16, None) == -1 and b"8192" in lib.df3d_last_error()
    assert pk(ctypes.c_void_p(4100), 1, 19, 64, 128, 4, p16, p16, p16, None) == -1 and b"16-byte" in lib.df3d_last_error()
    assert pk(None, 1, 19, 64, 128, 4, None, None, None, None) == -1 and b"null" in lib.df3d_last_error()
    assert pk(None, 0, 19, 64, 128, 4, None, None, None, None) == 0


def test_header_and_prototypes_list_the_new_entries(native_lib):
    import os
    import re

    from deepfly3d_amd import _native

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "df3d_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(df3d_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_native.PROTOTYPES)
    for name in ("df3d_heatmap_argmax_subpixel", "df3d_heatmap_peaks_subpixel"):
        assert name in declared and hasattr(native_lib, name)
    # same argument lists as the plain entries
    assert _native.PROTOTYPES["df3d_heatmap_argmax_subpixel"] == _native.PROTOTYPES["df3d_heatmap_argmax_checked"]
    assert _native.PROTOTYPES["df3d_heatmap_peaks_subpixel"] == _native.PROTOTYPES["df3d_heatmap_peaks"]
    assert native_lib.df3d_version() == 610   # additive: the revision stays


def test_cli_subpixel_flag():
    from deepfly3d_amd.cli import parse_cli_args

    assert parse_cli_args(["/tmp/x", "--subpixel"]).subpixel is True
    assert parse_cli_args(["/tmp/x"]).subpixel is False
    assert parse_cli_args(["/tmp/x", "--subpixel", "--auto-correct"]).subpixel is True
    with pytest.raises(SystemExit) as e:
        parse_cli_args(["/tmp/x", "--subpixel", "--skip-pose-estimation"])
    assert e.value.code == 2


def test_python_entries_refuse_cpu_tensors():
    torch = pytest.importorskip("torch")
    from deepfly3d_amd import ops

    with pytest.raises(ValueError):
        ops.heatmap_argmax(torch.zeros((1, 19, 64, 128)), subpixel=True)   # the kernels run on the device only
    with pytest.raises(ValueError):
        ops.heatmap_peaks(torch.zeros((1, 19, 64, 128)), 4, subpixel=True)
