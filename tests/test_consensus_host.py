"""CPU tests of the consensus triangulation's model (tests/consensus_oracle.py) and of the host-side refusals: no
kernel runs here.  What tests/test_gpu_consensus.py leans on is proved here, on the oracle alone."""
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest

import consensus_cases as cc
import consensus_oracle as co
import pose_chain_cases as pc
from oracle import geometry as og

NAN = float("nan")


def _keys(P, px_point, cand_X_point, X_full, tau, min_views):
    vm = co.view_mask(px_point)
    keys = []
    for mask in range(1 << px_point.shape[0]):
        if (vm & mask) != mask or len(co.cams_of(mask)) < max(min_views, 2):
            continue
        ok, size, sse = co.key_of(P, px_point, X_full if mask == vm else cand_X_point[mask], mask, tau)
        keys.append((mask, ok, size, sse))
    return vm, keys


@pytest.mark.parametrize("min_views", [2, 3, 8])
def test_the_choice_is_the_brute_force_maximum(min_views):
    """Every point of the staircase (0 .. 8 views), of a planted layout and of the special inputs: the oracle's choice is the one
    candidate that beats every other in pairwise comparison."""
    P = cc.rig()
    cases = [(P, cc.staircase(), 5.0), (P, cc.planted(8, 2)[0][:, :12], 5.0), (P, cc.planted(5, 1)[0][:, :20], 0.8), cc.special() + (5.0,)]
    seen = set()
    with np.errstate(all="ignore"):
        for P, px, tau in cases:
            cand, full = co.candidates(P, px), co.dlt(P, px)
            X, cameras, status, err, fixed, counts = co.choose(P, px, cand, full, tau, min_views)
            for i in range(px.shape[1]):
                vm, keys = _keys(P, px[:, i, 0], cand[i, 0], full[i, 0], tau, min_views)
                want = co.brute_force_choice(keys)
                n = len(co.cams_of(vm))
                if n < 2:
                    assert status[i, 0] == 0 and cameras[i, 0] == 0 and not X[i, 0].any() and not err[:, i, 0].any()
                elif want is None:
                    assert status[i, 0] == 3 and cameras[i, 0] == vm and np.array_equal(X[i, 0], full[i, 0], equal_nan=True)
                    assert np.array_equal(fixed[:, i, 0], px[:, i, 0], equal_nan=True)
                else:
                    assert cameras[i, 0] == want and status[i, 0] == (1 if want == vm else 2)
                    assert np.array_equal(X[i, 0], full[i, 0] if want == vm else cand[i, 0, want])
                if n < min_views:
                    assert status[i, 0] in (0, 3)
                seen.add(int(status[i, 0]))
            assert counts.sum() == px.shape[1] and np.array_equal(counts[0], np.bincount(status[:, 0], minlength=4))
    assert {0, 1, 3} <= seen and (2 in seen) == (min_views < 8)   # a proper subset of at most eight views holds fewer than eight


def test_the_order_is_total_and_needs_no_tolerance():
    """Size first, then the sum of squares, then the bitmask, compared as they are: a last-bit difference in sse decides."""
    one = 1.0 + 2.0 ** -52
    keys = [(0b0011, True, 2, 1.0), (0b0101, True, 2, 1.0), (0b0110, True, 2, one), (0b0111, False, 3, 0.0), (0b1001, True, 2, 0.5)]
    assert co.brute_force_choice(keys) == 0b1001
    assert co.brute_force_choice(keys[:4]) == 0b0011            # equal sse: the smaller bitmask
    assert co.brute_force_choice(keys[1:4]) == 0b0101           # 1.0 < 1 + 2^-52
    assert co.brute_force_choice(keys + [(0b1110, True, 3, 9.0)]) == 0b1110   # a larger set wins whatever its error
    assert co.brute_force_choice([keys[3]]) is None
    for perm in itertools.permutations(keys):
        assert co.brute_force_choice(list(perm)) == 0b1001


def test_the_normal_matrix_agrees_with_the_svd_at_every_subset_size():
    """The condition under the DLT bar of the GPU test: on the clean detections, all 247 subsets of the eight cameras."""
    P, px = cc.rig(), pc.detections()[0]
    worst = {}
    for k in range(2, 9):
        worst[k] = max(float(np.abs(pc.triangulate_eigh(only, P) - og.triangulate_dlt_batched(only, P)).max())
                       for only in (pc.only_cameras(px, s) for s in itertools.combinations(range(8), k)))
    print("worst |eigh - SVD| by subset size: " + ", ".join(f"{k}: {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= pc.TRI_CONDITION


def test_the_condition_holds_on_the_packed_clean_cases():
    """The same condition on every candidate of the launches whose points differ in their number of views (clean variants)."""
    for name, P, px in cc.packed_clean_cases():
        ncam, worst = px.shape[0], {}
        vm = sum(og.visibility(px[c]).astype(np.int64) << c for c in range(ncam))
        for mask in range(1 << ncam):
            cams = co.cams_of(mask)
            at = (vm & mask) == mask
            if len(cams) >= 2 and at.any():
                only = pc.only_cameras(px, cams)
                worst[len(cams)] = max(worst.get(len(cams), 0.0), float(np.abs(pc.triangulate_eigh(only, P) - co.dlt(P, only))[at].max()))
        print(f"{name}: worst |eigh - SVD| by subset size: " + ", ".join(f"{k}: {v:.1e}" for k, v in sorted(worst.items())))
        assert worst and max(worst.values()) <= pc.TRI_CONDITION, name


@pytest.mark.parametrize("layout", cc.CLEAN_LAYOUTS, ids=lambda l: f"{l[0]}views{l[1]}out")
def test_three_clean_views_recover_the_clean_set(layout):
    P = cc.rig()
    px, clean = cc.planted(*layout)
    X, cameras, status, err, fixed, counts = co.consensus(P, px, cc.TAU)
    inlier = max(err[c, i, 0] for i in range(px.shape[1]) for c in co.cams_of(int(clean[i])))
    print(f"{layout}: recovered {int((cameras[:, 0] == clean).sum())} of {px.shape[1]}, worst inlier error {inlier:.2f} px")
    assert np.array_equal(cameras[:, 0], clean) and (status == 2).all() and inlier < cc.TAU
    truth = pc.detections()[1]
    plain = og.triangulate_dlt_batched(px, P)[:, 0]
    assert np.linalg.norm(X[:, 0] - truth, axis=1).max() < np.linalg.norm(plain - truth, axis=1).max()
    # every rejected detection is replaced by a projection that lies within tau of the clean detection it was moved from
    moved = np.abs(fixed - pc.detections()[0][:, :, :, :]).max(axis=-1)[:layout[0]]
    assert moved.max() < cc.TAU


def test_two_clean_views_of_three_are_the_models_limit():
    """Three views, one outlier: the count is what the oracle gives -- the model cannot do better, and nothing here claims it does."""
    px, clean = cc.planted(*cc.AMBIGUOUS_LAYOUT)
    cameras = co.consensus(cc.rig(), px, cc.TAU)[1][:, 0]
    got = int((cameras == clean).sum())
    print(f"3 views, 1 outlier: the clean pair on {got} of {px.shape[1]} points")
    assert got == cc.AMBIGUOUS_RECOVERED < px.shape[1]


def test_infinite_tau_keeps_every_finite_point_and_zero_tau_none():
    P, px = cc.rig(), cc.staircase()
    cand, full = co.candidates(P, px), co.dlt(P, px)
    n = np.array([len(co.cams_of(co.view_mask(px[:, i, 0]))) for i in range(px.shape[1])])
    X, cameras, status, *_ = co.choose(P, px, cand, full, math.inf)
    assert np.array_equal(X, full) and np.array_equal(status[:, 0], np.where(n >= 2, 1, 0))
    X, cameras, status, *_ = co.choose(P, px, cand, full, 0.0)
    assert np.array_equal(X, full) and np.array_equal(status[:, 0], np.where(n >= 2, 3, 0))


# ------------------------------------------------------------------------------------------------------------------ host refusals
def test_consensus_params():
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops

    t, m = ops.consensus_params()
    assert t.dtype == np.float64 and np.array_equal(t, np.full(38, 20.0)) and np.array_equal(t, cfg.ROBUST_TAU) and t is not cfg.ROBUST_TAU
    assert m == cfg.ROBUST_MIN_VIEWS == 2
    t, m = ops.consensus_params(5, 8)
    assert t.tolist() == [5.0] and m == 8
    assert ops.consensus_params(np.arange(38.0), np.int64(3))[0].shape == (38,)
    assert ops.consensus_params(math.inf)[0].tolist() == [math.inf] and ops.consensus_params(0.0)[0].tolist() == [0.0]
    for bad in (-1.0, NAN, [1.0, -2.0], [1.0, NAN], [], "5", True, object(), [None]):
        with pytest.raises(ValueError, match="tau must be"):
            ops.consensus_params(bad)
    for bad in (1, 9, 0, -2, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"min_views must be an integer in \[2, 8\]"):
            ops.consensus_params(None, bad)
    assert list(inspect.signature(ops.consensus_params).parameters) == ["tau", "min_views"]
    assert list(inspect.signature(ops.consensus_candidates).parameters) == ["P", "points2d_px", "X"]
    assert list(inspect.signature(ops.triangulate_consensus).parameters) == ["P", "points2d_px", "X", "tau", "min_views"]
    assert [f.name for f in ops.ConsensusResult.__dataclass_fields__.values()] == ["points3d", "cameras", "status", "error", "fixed_px", "counts",
                                                                                   "params"]


def _one_frame_folder(tmp_path, golden_dir):
    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    return str(folder)


def test_core_refusals_and_keys(tmp_path, golden_dir):
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    assert Core._ROBUST_KEYS == ("points3d_robust", "robust_cameras", "robust_status", "robust_error", "robust_counts", "points2d_robust",
                                 "robust_params")
    names = list(inspect.signature(Core.save).parameters)
    assert names[-3:] == ["robust_triangulation", "robust_tau", "robust_min_views"]
    defaults = [inspect.signature(Core.save).parameters[n].default for n in names[-3:]]
    assert defaults == [False, None, None]
    assert list(inspect.signature(Core.robust_triangulation).parameters) == ["self", "tau", "min_views"]
    assert list(inspect.signature(Core.outlier_cameras).parameters) == ["self", "img_id", "joint_id"]
    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    with pytest.raises(RuntimeError, match="robust_triangulation needs calibrated cameras"):
        core.robust_triangulation()
    with pytest.raises(RuntimeError, match="outlier_cameras needs calibrated cameras"):
        core.outlier_cameras(0)
    with pytest.raises(ValueError, match="tau must be"):   # before the cameras are asked for
        core.robust_triangulation(tau=-1.0)
    with pytest.raises(ValueError, match="min_views must be"):
        core.robust_triangulation(min_views=1)
    for option in ("robust_tau", "robust_min_views"):
        with pytest.raises(ValueError, match="robust_tau and robust_min_views belong to robust_triangulation"):
            core.save(**{option: 3})
    with pytest.raises(ValueError, match="tau must be"):
        core.save(robust_triangulation=True, robust_tau=NAN)
    with pytest.raises(ValueError, match="min_views must be"):
        core.save(robust_triangulation=True, robust_min_views=9)
    with pytest.raises(ValueError, match="robust_tau must hold one value, or one per joint"):
        core.save(robust_triangulation=True, robust_tau=[1.0, 2.0])
    assert not [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]
    config.pop("image_shape", None)


def test_cli_options_and_refusals(capsys, tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    for argv, message in ((["x", "--robust-tau", "5"], "--robust-tau sets a parameter of --robust-triangulation"),
                          (["x", "--robust-min-views", "3"], "--robust-min-views sets a parameter of --robust-triangulation"),
                          (["x", "--robust-triangulation", "--robust-tau=-1"], "tau must be >= 0 and not NaN"),
                          (["x", "--robust-triangulation", "--robust-tau", "nan"], "tau must be >= 0 and not NaN"),
                          (["x", "--robust-triangulation", "--robust-min-views", "1"], r"min_views must be an integer in \[2, 8\]"),
                          (["x", "--robust-triangulation", "--robust-min-views", "9"], r"min_views must be an integer in \[2, 8\]")):
        with pytest.raises(SystemExit):
            cli.parse_cli_args(argv)
        assert re.search(message, capsys.readouterr().err), argv
    args = cli.parse_cli_args(["x", "--robust-triangulation", "--robust-tau", "7.5", "--robust-min-views", "3", "--skip-pose-estimation"])
    assert args.robust_triangulation and args.robust_tau == 7.5 and args.robust_min_views == 3
    args = cli.parse_cli_args(["x"])
    assert not args.robust_triangulation and args.robust_tau is None and args.robust_min_views is None
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--robust-tau PX" in text and "--robust-min-views N" in text and "a guess that nobody has measured on a recording" in text
    assert "near an epipolar line" in text
    folder = _one_frame_folder(tmp_path, golden_dir)
    config.pop("image_shape", None)
    with pytest.raises(RuntimeError, match="--robust-triangulation needs calibrated cameras"):
        cli.run(cli.parse_cli_args([folder, "--robust-triangulation", "--skip-pose-estimation"]))
    config.pop("image_shape", None)
