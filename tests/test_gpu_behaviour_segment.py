"""GPU tests of the behaviour map's segmentation: csrc/behaviour_segment.hip against the float64 oracle of
tests/behaviour_segment_oracle.py.  Only the density carries a floating-point bar, derived there; every integer output -- regions,
roots, labels, bouts, occupancy, transitions -- is compared exactly, the watershed teacher-forced on the device's own density."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import behaviour_segment_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_SIGMA = 0.02   # far cells underflow to exact 0


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)   # a copy: the shared references are read-only


@functools.lru_cache(maxsize=None)
def _reference(M, T, G, sigma):
    """(Y, origin, sigma, rho, A) of one density case: computed once, shared, never changed."""
    Y = bo.density_case(M, T)
    origin, sigma = bo.grid(Y, G, sigma)
    rho, A = bo.density(Y, origin, sigma, G)
    for a in (Y, rho, A):
        a.setflags(write=False)
    return Y, origin, sigma, rho, A


def _sigmas(M):
    return (None if M > 1 else 1.0, SMALL_SIGMA)   # one frame has no extent and so no default sigma: it gets 1


# ------------------------------------------------------------------------------------------------------------------ density
@pytest.mark.parametrize("M,T,G", bo.DENSITY_CASES)
def test_density_and_teacher_forced_watershed(native_lib, cuda, M, T, G):
    """One block and one slice, a ragged tile, more tiles than one, a ragged slice, two slices; invalid rows spread through the
    input.  Then the device's own density through the watershed, against the oracle's on the same array, exactly."""
    from deepfly3d_amd import ops

    assert native_lib.df3d_bseg_work_bytes(3 * bo.DENSITY_SLICE + 1, 256) - native_lib.df3d_bseg_work_bytes(3 * bo.DENSITY_SLICE, 256) == 8 * 256 ** 2
    for sigma_arg in _sigmas(M):
        Y, origin, sigma, want, A = _reference(M, T, G, sigma_arg)
        rho, got_origin, got_sigma = ops.map_density(_dev(Y, cuda), G, sigma_arg)
        assert got_origin == origin and got_sigma == sigma and rho.shape == (G, G) and rho.dtype == torch.float64
        got = rho.cpu().numpy()
        bar = bo.density_tolerance(want, A, M)
        err = np.abs(got - want)
        print(f"M = {M} of {T}, G = {G}, sigma = {sigma:.4g}: max |device - oracle| / bar = {float((err / bar).max()):.3g}; "
              f"{int((want == 0).sum())} cells exactly 0 in the oracle, the device's largest there {float(np.abs(got[want == 0]).max()) if (want == 0).any() else 0.0:.3g}")
        assert np.isfinite(got).all() and np.all(got >= 0)
        assert np.all(err <= bar)
        assert np.all(got[want == 0] < 2.3e-308)   # 0 or denormal
        if M > 1 and sigma_arg == SMALL_SIGMA:
            assert (want == 0).any()
        for min_peak in (None, 0.0, 0.3):
            regions, roots = ops.watershed(rho, min_peak)
            w_regions, R, w_roots, _ = bo.watershed(got, bo.MIN_PEAK if min_peak is None else min_peak)
            assert regions.dtype == roots.dtype == torch.int32 and roots.shape == (R,)
            assert np.array_equal(regions.cpu().numpy(), w_regions) and np.array_equal(roots.cpu().numpy(), w_roots)
        # labels of the same frames in the device's regions (min_peak 0.3), and their ethogram
        lab = ops.map_labels(_dev(Y, cuda), regions, origin)
        w_lab = bo.labels(Y, w_regions, origin)
        assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), w_lab) and (w_lab == -1).sum() == T - M
        for g, w in zip(ops.ethogram(lab, R), bo.ethogram(w_lab, R)):
            assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w)


# ------------------------------------------------------------------------------------------------------------------ watershed
def test_watershed_on_built_fields(native_lib, cuda):
    from deepfly3d_amd import ops

    for name, (rho, min_peak) in bo.built_fields().items():
        regions, roots = ops.watershed(_dev(rho, cuda), min_peak)
        want, R, w_roots, longest = bo.watershed(rho, min_peak)
        assert np.array_equal(regions.cpu().numpy(), want), name
        assert np.array_equal(roots.cpu().numpy(), w_roots) and len(w_roots) == R, name
        if name == "spiral ridge":
            assert longest > rho.shape[0]   # a chain longer than G: log2 G doubling rounds would leave it short


# ------------------------------------------------------------------------------------------------------------------ labels, ethogram
def test_labels_on_cell_edges_and_the_outer_border(native_lib, cuda):
    from deepfly3d_amd import ops

    origin = (-2.0, 10.0, 0.5)
    regions = np.arange(1, 17, dtype=np.int32).reshape(4, 4)
    Y = np.array([[-2.0, 10.0], [-1.5, 10.0], [-1.5000000000000002, 10.5], [0.0, 12.0], [5.0, 99.0], [-7.0, 9.999], [-0.5, 11.5],
                  [np.nan, 10.0], [-1.0, np.inf], [-1e308, 1e308]])
    got = ops.map_labels(_dev(Y, cuda), _dev(regions, cuda), origin).cpu().numpy()
    assert list(got) == [1, 2, 5, 16, 16, 1, 16, -1, -1, 13] and np.array_equal(got, bo.labels(Y, regions, origin))


@pytest.mark.parametrize("T", bo.SCAN_SIZES)
def test_labels_and_ethogram_sizes(native_lib, cuda, T):
    """Across the scan's block edge (256) and its block-of-blocks edge (256 * 256): frames through the labels kernel, and synthetic
    label rows -- random runs, one bout, a change at every frame -- through the ethogram."""
    from deepfly3d_amd import ops

    rng = np.random.default_rng(T)
    G, origin = 7, (-1.0, 2.0, 0.25)
    regions = rng.integers(0, 6, size=(G, G)).astype(np.int32)
    Y = rng.uniform(-1.5, 1.5, size=(T, 2)) + (0.0, 3.0)
    Y[rng.random(T) < 0.05, 0] = np.nan
    lab = ops.map_labels(_dev(Y, cuda), _dev(regions, cuda), origin)
    want = bo.labels(Y, regions, origin)
    assert np.array_equal(lab.cpu().numpy(), want)
    rows = [want] + [bo.label_row(T, kind) for kind in ("random", "single", "alternating")]
    for row in rows:
        got = ops.ethogram(_dev(row, cuda), 5)
        w_bouts, w_occ, w_tr = bo.ethogram(row, 5)
        assert got[0].shape == w_bouts.shape and got[0].dtype == torch.int64
        assert np.array_equal(got[0].cpu().numpy(), w_bouts) and np.array_equal(got[1].cpu().numpy(), w_occ) and np.array_equal(got[2].cpu().numpy(), w_tr)
        assert int(got[0][:, 2].sum()) == T
    assert len(bo.ethogram(rows[2], 5)[0]) == 1 and len(bo.ethogram(rows[3], 5)[0]) == T
    # more labels than the counting kernel keeps in LDS (32): the tables are counted in global memory
    many = bo.label_row(T, "random", R=40)
    for g, w in zip(ops.ethogram(_dev(many, cuda), 40), bo.ethogram(many, 40)):
        assert np.array_equal(g.cpu().numpy(), w)


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_determinism_guard_words_and_a_side_stream(native_lib, cuda):
    """The raw entries on sentinel-filled buffers inside guard words, the workspace too, on a stream of their own: two runs are
    bit-equal, every output element is written and nothing outside is."""
    lib = native_lib
    M, T, G = bo.DENSITY_CASES[-1]   # two slices, four tiles
    Y, origin, sigma, want, A = _reference(M, T, G, None)
    GUARD, n = 64, G * G
    need = lib.df3d_bseg_work_bytes(T, G)
    assert need % 16 == 0
    side = torch.cuda.Stream(device=cuda)
    st = side.cuda_stream
    fills = {torch.float64: -1.2345e30, torch.int32: -77, torch.int64: -7777}

    def guarded(count, dtype=torch.float64):
        t = torch.full((count + 2 * GUARD,), fills[dtype], dtype=dtype, device=cuda)
        return t, t.data_ptr() + GUARD * t.element_size()

    def inner(t):
        a = t.cpu().numpy()
        fill = fills[t.dtype]
        assert np.all(a[:GUARD] == fill) and np.all(a[-GUARD:] == fill), "a guard word was written"
        return a[GUARD:-GUARD]

    runs = []
    with torch.cuda.stream(side):
        Yd = _dev(Y, cuda)
        for _ in range(2):
            bounds, rho, regions, count, roots = guarded(5), guarded(n), guarded(n, torch.int32), guarded(1, torch.int32), guarded(n, torch.int32)
            labels, bouts, nb = guarded(T, torch.int32), guarded(3 * T, torch.int64), guarded(1, torch.int32)
            work = guarded(need // 8)
            for rc in (lib.df3d_bseg_bounds(Yd.data_ptr(), T, bounds[1], st),
                       lib.df3d_bseg_density(Yd.data_ptr(), T, *origin, G, sigma, rho[1], work[1], need, st),
                       lib.df3d_bseg_watershed(rho[1], G, 0.0, regions[1], count[1], roots[1], work[1], need, st),
                       lib.df3d_bseg_labels(Yd.data_ptr(), T, *origin, G, regions[1], labels[1], st)):
                assert rc == 0, lib.df3d_last_error()
            side.synchronize()
            R = int(inner(count[0])[0])
            occ, tr = guarded(R + 1, torch.int64), guarded((R + 1) ** 2, torch.int64)
            assert lib.df3d_bseg_bouts(labels[1], T, R, bouts[1], nb[1], occ[1], tr[1], work[1], need, st) == 0, lib.df3d_last_error()
            side.synchronize()
            inner(work[0])
            runs.append({k: inner(v[0]).copy() for k, v in dict(bounds=bounds, rho=rho, regions=regions, count=count, roots=roots, labels=labels,
                                                                bouts=bouts, nb=nb, occ=occ, tr=tr).items()})
    first, second = runs
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), f"{k} differs between two runs"
        assert not np.any(first[k] == fills[torch.from_numpy(first[k]).dtype]), f"{k} was not written everywhere"
    v = Y[bo.valid_rows(Y)]
    assert list(first["bounds"]) == [v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max(), float(M)]
    rho = first["rho"].reshape(G, G)
    assert np.all(np.abs(rho - want) <= bo.density_tolerance(want, A, M))
    w_regions, R, w_roots, _ = bo.watershed(rho, 0.0)
    assert first["count"][0] == R and np.array_equal(first["regions"].reshape(G, G), w_regions)
    assert np.array_equal(first["roots"][:R], w_roots) and np.all(first["roots"][R:] == -1)
    w_lab = bo.labels(Y, w_regions, origin)
    w_bouts, w_occ, w_tr = bo.ethogram(w_lab, R)
    B = int(first["nb"][0])
    assert np.array_equal(first["labels"], w_lab) and B == len(w_bouts)
    assert np.array_equal(first["bouts"].reshape(T, 3)[:B], w_bouts) and not first["bouts"].reshape(T, 3)[B:].any()
    assert np.array_equal(first["occ"], w_occ) and np.array_equal(first["tr"].reshape(R + 1, R + 1), w_tr)


# ------------------------------------------------------------------------------------------------------------------ the planted case
@pytest.mark.parametrize("G", bo.PLANTED["grids"])
def test_planted_case(native_lib, cuda, G):
    """Three planted behaviours, an outlier and two NaN rows: no frame is excused."""
    from deepfly3d_amd import ops

    Y, behaviour = bo.planted_case()
    for min_peak in (bo.PLANTED["keep_three"], bo.PLANTED["keep_four"]):
        s = ops.segment_map(_dev(Y, cuda), G, bo.PLANTED["sigma"], min_peak)
        lab, R = s.labels.cpu().numpy(), s.region_peaks.shape[0]
        bo.check_planted(lab, R, behaviour, min_peak)
        want = bo.segment(Y, G, bo.PLANTED["sigma"], min_peak)
        assert s.origin == want["origin"] and s.sigma == want["sigma"]
        # the oracle's chain on the device's density: everything downstream is exact
        regions, R2, roots, _ = bo.watershed(s.density.cpu().numpy(), min_peak)
        assert R2 == R and np.array_equal(s.regions.cpu().numpy(), regions)
        gx, gy = bo.centres(s.origin, G)
        assert np.array_equal(s.region_peaks.cpu().numpy(), np.stack((gx[roots % G], gy[roots // G]), axis=1))
        assert np.array_equal(lab, bo.labels(Y, regions, s.origin))
        for g, w in zip((s.bouts, s.occupancy, s.transitions), bo.ethogram(lab, R)):
            assert np.array_equal(g.cpu().numpy(), w)
        assert np.array_equal(lab, want["labels"]) and R == want["R"]   # and here the oracle's own density gives the same regions


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_segment_map_shapes_through_ops(native_lib, cuda):
    from deepfly3d_amd import ops

    Y, _ = bo.planted_case(1)
    plain = ops.segment_map(_dev(Y, cuda), 33, 1.5, 0.1)
    wide = _dev(np.repeat(Y, 2, axis=1), cuda)[:, ::2]   # not contiguous: ops copies
    assert not wide.is_contiguous()
    again = ops.segment_map(wide, 33, 1.5, 0.1)
    for a, b in zip(plain, again):
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    assert plain.density.shape == (33, 33) and plain.regions.shape == (33, 33) and plain.labels.shape == (120,)
    assert plain.region_peaks.shape == (3, 2) and plain.occupancy.shape == (4,) and plain.transitions.shape == (4, 4)
    assert plain.bouts.shape[1] == 3 and int(plain.bouts[:, 2].sum()) == 120
    default = ops.segment_map(_dev(Y, cuda))
    assert default.density.shape == (256, 256) and default.sigma == bo.grid(Y)[1]
    with pytest.raises(ValueError, match="no valid frame"):
        ops.segment_map(torch.zeros((0, 2), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="no valid frame"):
        ops.segment_map(torch.full((5, 2), float("nan"), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="lies on one point"):
        ops.segment_map(torch.ones((5, 2), dtype=torch.float64, device=cuda))
    one = ops.segment_map(torch.ones((5, 2), dtype=torch.float64, device=cuda), 8, sigma=0.5)
    # the point sits on the corner four cells share: whichever of them is the root, its region holds the point
    assert one.region_peaks.shape[0] >= 1 and int(one.labels[0]) >= 1
    assert int(one.occupancy.sum()) == 5 and one.bouts.cpu().numpy().tolist() == [[int(one.labels[0]), 0, 5]]
    with pytest.raises(ValueError, match=r"grid must be an integer in \[2, 1024\]"):
        ops.segment_map(_dev(Y, cuda), 1)
    with pytest.raises(ValueError, match=r"min_peak must be in \[0, 1\]"):
        ops.segment_map(_dev(Y, cuda), 16, 1.5, 1.5)
    empty = ops.ethogram(torch.zeros((0,), dtype=torch.int32, device=cuda), 2)
    assert empty[0].shape == (0, 3) and empty[1].tolist() == [0, 0, 0] and not empty[2].any()
    assert ops.map_labels(torch.zeros((0, 2), dtype=torch.float64, device=cuda), plain.regions, plain.origin).shape == (0,)


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


SEGMENT_KEYS = ["behaviour_density", "behaviour_density_origin", "behaviour_density_sigma", "behaviour_regions", "behaviour_region_peaks",
                "behaviour_labels", "behaviour_bouts", "behaviour_occupancy", "behaviour_transitions"]


def _check_segments(run, tag, G, sigma_arg=None):
    """The nine keys of one map against the oracle's chain on the stored map; everything after the density exactly."""
    Y = run["behaviour_map" + tag]
    k = {name[len("behaviour_"):]: run[name + tag] for name in SEGMENT_KEYS}
    origin, sigma = tuple(k["density_origin"]), k["density_sigma"]
    assert k["density_origin"].shape == (3,) and isinstance(sigma, float)
    assert (origin, sigma) == bo.grid(Y, G, sigma_arg)
    want, A = bo.density(Y, origin, sigma, G)
    M = int(bo.valid_rows(Y).sum())
    assert k["density"].shape == (G, G) and np.all(np.abs(k["density"] - want) <= bo.density_tolerance(want, A, M))
    lab = k["labels"]
    assert lab.dtype == np.int32 and lab.shape == (15,) and k["regions"].dtype == np.int32 and k["regions"].shape == (G, G)
    assert np.array_equal(lab, bo.labels(Y, k["regions"], origin))   # the labels, recomputed on the host from the stored regions and map
    assert np.array_equal(lab == -1, ~bo.valid_rows(Y))
    R = int(k["regions"].max())
    assert k["region_peaks"].shape == (R, 2) and R >= 1
    for got, w in zip((k["bouts"], k["occupancy"], k["transitions"]), bo.ethogram(lab, R)):
        assert got.dtype == np.int64 and np.array_equal(got, w)
    return k


def test_core_behaviour_segments(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    m = core.behaviour_map(perplexity=4)
    s = core.behaviour_segments(grid=48, min_peak=0.05, perplexity=4)
    assert isinstance(s, ops.BehaviourSegmentsResult) and all(isinstance(a, np.ndarray) for a in (s.density, s.regions, s.region_peaks, s.labels,
                                                                                                 s.bouts, s.occupancy, s.transitions))
    run = {"behaviour_map": m.embedding, **{name: value for name, value in zip(SEGMENT_KEYS, (s.density, np.array(s.origin), s.sigma, s.regions,
                                                                                                  s.region_peaks, s.labels, s.bouts, s.occupancy,
                                                                                                  s.transitions))}}
    _check_segments(run, "", 48)
    regions, R, roots, _ = bo.watershed(s.density, 0.05)
    assert np.array_equal(s.regions, regions) and s.region_peaks.shape == (R, 2)
    with pytest.raises(ValueError, match="perplexity 32 needs at least 97 frames"):
        core.behaviour_segments()
    with pytest.raises(ValueError, match="needs behaviour_map=True"):
        core.save(behaviour_segments=True)
    with pytest.raises(ValueError, match="need behaviour_segments=True"):
        core.save(behaviour_map=True, behaviour_perplexity=4, behaviour_grid=32)
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_behaviour_segments(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    with open(pkl, "rb") as f:
        earlier = f.read()
    order = [str(c) for c in range(7)]

    def reopen(*flags):
        with open(pkl, "wb") as f:
            f.write(earlier)
        assert cli.main([folder, "--skip-pose-estimation", *flags, "--order"] + order) == 0
        return _load(pkl)

    base = ("--behaviour-map", "--behaviour-perplexity", "4")
    for rigid in ((), ("--rigid-legs",)):
        before = reopen(*base, *rigid)
        run = reopen(*base, "--behaviour-segments", *rigid)
        tags = ("", "_rigid") if rigid else ("",)
        assert list(run.keys()) == list(before.keys()) + [k + tag for tag in tags for k in SEGMENT_KEYS]
        assert all(_same(before[k], run[k]) for k in before)   # every earlier key byte for byte
        for tag in tags:
            _check_segments(run, tag, bo.GRID)
    small = reopen(*base, "--behaviour-segments", "--behaviour-grid", "32", "--behaviour-sigma", "40")
    _check_segments(small, "", 32, 40.0)
    assert small["behaviour_density"].shape == (32, 32) and small["behaviour_density_sigma"] == 40.0
    assert _same(small["behaviour_map"], run["behaviour_map"])
    regions, R, roots, _ = bo.watershed(small["behaviour_density"], bo.MIN_PEAK)
    assert np.array_equal(small["behaviour_regions"], regions) and small["behaviour_region_peaks"].shape == (R, 2)
    assert np.array_equal(small["behaviour_labels"], bo.labels(small["behaviour_map"], regions, tuple(small["behaviour_density_origin"])))
    with open(pkl, "wb") as f:
        f.write(earlier)
    with pytest.raises(SystemExit):
        cli.main([folder, "--skip-pose-estimation", "--behaviour-segments", "--order"] + order)
    with open(pkl, "rb") as f:
        assert f.read() == earlier   # refused before any work: the earlier result is untouched
    config.pop("image_shape", None)
