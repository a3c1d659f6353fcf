"""GPU tests of the pictorial-structures correction against the float64 oracle tests/pictorial_oracle.py:
heat-map peaks bit for bit, proposals and the exact solve to 1e-9, a planted-distractor scenario on the golden recording, and
the pipeline surface (inference_folder(return_peaks=K), Core.auto_correct, df3d-cli --auto-correct on one and two ranks)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import pictorial_oracle as po

pytestmark = pytest.mark.gpu

ORDER = [0, 1, 2, 3, 4, 5, 6]
IMAGE_SHAPE = [960, 480]   # [W, H]


def _cams(golden_dir):
    from oracle import geometry as og

    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    return og.projection_matrices(g3["R"], g3["tvec"], g3["intr"]), g3


def _peaks_dev(hm, k, cuda):
    from deepfly3d_amd import ops

    c, p, v = ops.heatmap_peaks(torch.from_numpy(np.ascontiguousarray(hm)).to(cuda), k)
    return c.cpu().numpy(), p.cpu().numpy(), v.cpu().numpy()


def _argmax_dev(hm, cuda):
    from deepfly3d_amd import ops

    p, c = ops.heatmap_argmax(torch.from_numpy(np.ascontiguousarray(hm)).to(cuda))
    return p.cpu().numpy(), c.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ peaks
@pytest.mark.parametrize("k", [1, 10, 16])
def test_peaks_random_planes_bit_exact(native_lib, cuda, k):
    rng = np.random.default_rng(k)
    hm = rng.standard_normal((3, 19, 64, 128)).astype(np.float32)
    hm[1] = np.round(hm[1] * 2) / 2   # coarse values: ties between peaks and plateaus
    got = _peaks_dev(hm, k, cuda)
    want = po.heatmap_peaks(hm, k)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    pts, conf = _argmax_dev(hm, cuda)
    assert np.array_equal(got[1][:, :, 0], pts) and np.array_equal(got[2][:, :, 0], conf)


def test_peaks_special_planes_bit_exact(native_lib, cuda):
    rng = np.random.default_rng(5)
    planes = []
    planes.append(np.zeros((64, 128), np.float32))                                  # constant
    planes.append(np.full((64, 128), 3.5, np.float32))
    planes.append(rng.integers(0, 3, size=(64, 128)).astype(np.float32))           # plateaus and ties everywhere
    p = rng.random((64, 128)).astype(np.float32) * 0.5
    p[0, 0] = p[0, 127] = p[63, 0] = p[63, 127] = 2.0                                # corners
    p[0, 60] = p[63, 61] = p[30, 0] = p[31, 127] = 1.5                              # edges
    planes.append(p)
    p = rng.random((64, 128)).astype(np.float32)
    p[rng.random((64, 128)) < 0.05] = np.nan                                        # NaN cells
    planes.append(p)
    p = rng.random((64, 128)).astype(np.float32)
    p[10, 10], p[20, 20], p[30, 30] = np.inf, -np.inf, np.nan                       # +inf is never a peak, neighbours ignore it
    planes.append(p)
    planes.append(np.full((64, 128), np.nan, np.float32))                            # no peak at all
    planes.append(np.full((64, 128), -np.inf, np.float32))
    p = np.zeros((64, 128), np.float32)
    p[5:9, 40:50] = 1.0                                                              # a flat-topped peak: its first cell only
    p[40, 100] = p[40, 101] = 1.0                                                    # two equal cells side by side
    planes.append(p)
    hm = np.stack(planes)[None].repeat(2, axis=0)
    hm[1] = -hm[1]
    for k in (1, 10, 16):
        got = _peaks_dev(hm, k, cuda)
        want = po.heatmap_peaks(hm, k)
        for g, w in zip(got, want):
            assert np.array_equal(g, w, equal_nan=True)
        pts, conf = _argmax_dev(hm, cuda)
        comparable = (got[0] > 0) & ~np.isposinf(hm).any(axis=(2, 3))   # the arg-max is a peak when the maximum is finite
        assert comparable.sum() == 12   # 6 of the 9 planes per side hold a finite maximum
        assert np.array_equal(got[1][:, :, 0][comparable], pts[comparable]) and np.array_equal(got[2][:, :, 0][comparable], conf[comparable])


# ------------------------------------------------------------------------------------------------------------------ DLT move
def test_triangulate_bit_identical_to_before_the_dlt_move(native_lib, cuda, golden_dir):
    """triangulate_bits.npz holds df3d_triangulate's output from the build before the DLT code moved into geometry_dev.h."""
    from deepfly3d_amd import ops

    f = np.load(f"{golden_dir}/triangulate_bits.npz")
    for case in ("golden", "random"):
        X = ops.triangulate(f["P"], torch.from_numpy(f[f"{case}_px"]).to(cuda)).cpu().numpy()
        assert np.array_equal(X.view(np.uint64), f[f"{case}_X"].view(np.uint64)), case


# ------------------------------------------------------------------------------------------------------------------ proposals, solve
def _random_problem(golden_dir, T=3, k=10, seed=0):
    """Peaks scattered around the golden pose's projections (in network orientation) with random counts and values."""
    from deepfly3d_amd.synthetic import synthetic_points2d

    P, g3 = _cams(golden_dir)
    rng = np.random.default_rng(seed)
    clean = synthetic_points2d(g3["points3d_wo_procrustes"][:T], g3["R"], g3["tvec"], g3["intr"])   # [7, T, 38, 2] normalised
    table = po.seeing_table(ORDER)
    count = np.zeros((7, T, 19), np.int32)
    pts = np.zeros((7, T, 19, k, 2), np.float32)
    vals = np.zeros((7, T, 19, k), np.float32)
    for j in range(38):
        for c, src, left in table[j]:
            for t in range(T):
                n = int(rng.integers(1, k + 1))
                r0, c0 = clean[c, t, j, 0] * 64, (1 - clean[c, t, j, 1] if left else clean[c, t, j, 1]) * 128
                rr = np.clip(np.round(r0 + rng.normal(0, 4, n) * (np.arange(n) > 0)), 1, 63)
                cc = np.clip(np.round(c0 + rng.normal(0, 8, n) * (np.arange(n) > 0)), 1, 127)
                v = np.sort(rng.uniform(0.2, 1.0, n))[::-1]
                count[c, t, src] = n
                pts[c, t, src, :n, 0] = rr.astype(np.float32) * np.float32(1 / 64)
                pts[c, t, src, :n, 1] = cc.astype(np.float32) * np.float32(1 / 128)
                vals[c, t, src, :n] = v
    return P, count, pts, vals


def _to(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _argmax2d(pts, cuda):
    from deepfly3d_amd import ops

    return ops.relayout_19_to_38(torch.from_numpy(np.ascontiguousarray(pts[:, :, :, 0])).to(cuda), ORDER)


def test_proposals_and_solve_match_the_oracle(native_lib, cuda, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import bone_tree

    k, m = 10, 24
    P, count, pts, vals = _random_problem(golden_dir, T=3, k=k, seed=1)
    am = _argmax2d(pts, cuda)
    dc, dp, dv = _to(cuda, count, pts, vals)
    kept = ops.ps_proposals(P, ORDER, am, dc, dp, dv, IMAGE_SHAPE, num_proposals=m)
    kept = {n: t.cpu().numpy() for n, t in kept.items()}
    amh = am.cpu().numpy()
    ora = po.proposals(P, ORDER, amh, count, pts, vals, IMAGE_SHAPE, k, m)
    # proposal 0 is df3d_triangulate's point for the arg-max detections, bit for bit
    X0 = ops.triangulate(P, am * torch.tensor([480.0, 960.0], dtype=torch.float64, device=cuda)).cpu().numpy()
    assert np.array_equal(kept["X"][:, :, 0].view(np.uint64), X0.view(np.uint64))
    n_checked = 0
    for t in range(3):
        for j in range(38):
            o = ora["kept"][t][j]
            n = kept["count"][t, j]
            assert n == len(o["index"]), (t, j)
            assert np.array_equal(kept["index"][t, j, :n], o["index"]), (t, j)
            assert np.array_equal(kept["match"][t, j, :n], o["match"]), (t, j)
            scale = np.maximum(np.abs(o["U"]), 1.0)
            assert np.all(np.abs(kept["U"][t, j, :n] - o["U"]) <= 1e-9 * scale), (t, j)
            assert np.allclose(kept["X"][t, j, :n], o["X"], rtol=1e-9, atol=1e-9), (t, j)
            n_checked += n
    assert n_checked > 3 * 38 * 10
    # the solve on those kept sets
    parent, bone = bone_tree()
    pts2, choice, energy = (x.cpu().numpy() for x in ops.ps_solve(ORDER, am, dc, dp, ops.ps_proposals(P, ORDER, am, dc, dp, dv, IMAGE_SHAPE, num_proposals=m)))
    o_pts, o_choice, o_energy, margin = po.solve(ora["kept"], ORDER, amh, count, pts, parent, bone)
    assert np.all(np.abs(energy - o_energy) <= 1e-9 * np.maximum(np.abs(o_energy), 1.0))
    clear = margin > 1e-9
    assert clear.mean() > 0.5   # two-camera joints tie exactly: proposal 0 and pair proposal (0, 0) are the same DLT
    assert np.array_equal(choice[clear], o_choice[clear])
    same = (choice == o_choice)
    assert np.array_equal(pts2.transpose(1, 2, 0, 3)[same], o_pts.transpose(1, 2, 0, 3)[same])
    # the chunked driver gives the same answer as one chunk
    res = ops.pictorial_correct(P, ORDER, am, dc, dp, dv, IMAGE_SHAPE, num_proposals=m, chunk_frames=2)
    assert np.array_equal(res.points2d.cpu().numpy(), pts2) and np.array_equal(res.choice.cpu().numpy(), choice)
    assert np.array_equal(res.energy.cpu().numpy(), energy)


# ------------------------------------------------------------------------------------------------------------------ scenario
SIGMA = 1.5       # cells
MARGIN_U = 0.25   # the clean proposal beats every distractor proposal (with clean neighbours' bones) by at least this
MOVE_MM = 0.05    # the arg-max DLT of every distracted joint moves by more than this


def _gauss(r0, c0, h=1.0):
    r, c = np.mgrid[0:64, 0:128]
    return (h * np.exp(-((r - r0) ** 2 + (c - c0) ** 2) / (2 * SIGMA**2))).astype(np.float32)


def _render(golden_dir, T=15):
    """Gaussian heat-maps [7, T, 19, 64, 128] at the projected golden joints, in network orientation (left cameras flipped)."""
    from deepfly3d_amd.synthetic import synthetic_points2d

    P, g3 = _cams(golden_dir)
    clean = synthetic_points2d(g3["points3d_wo_procrustes"][:T], g3["R"], g3["tvec"], g3["intr"])
    hm = np.zeros((7, T, 19, 64, 128), np.float32)
    cell = {}
    for j, see in enumerate(po.seeing_table(ORDER)):
        for c, src, left in see:
            for t in range(T):
                r0 = int(round(clean[c, t, j, 0] * 64))
                c0 = int(round((1 - clean[c, t, j, 1] if left else clean[c, t, j, 1]) * 128))
                hm[c, t, src] = _gauss(r0, c0)
                cell[(c, t, j)] = (r0, c0)
    return P, hm, cell


def _run(P, hm, cuda, k=10, m=64):
    from deepfly3d_amd import ops

    T = hm.shape[1]
    h = torch.from_numpy(hm.reshape(7 * T, 19, 64, 128)).to(cuda)
    c, p, v = ops.heatmap_peaks(h, k)
    c, p, v = c.view(7, T, 19), p.view(7, T, 19, k, 2), v.view(7, T, 19, k)
    ap, _ = ops.heatmap_argmax(h)
    am = ops.relayout_19_to_38(ap.view(7, T, 19, 2).contiguous(), ORDER)
    res = ops.pictorial_correct(P, ORDER, am, c, p, v, IMAGE_SHAPE, num_proposals=m)
    px = torch.tensor([480.0, 960.0], dtype=torch.float64, device=cuda)
    return am, res, ops.triangulate(P, am * px), ops.triangulate(P, res.points2d * px), (c, p, v)


def test_scenario_clean_maps_are_left_alone(native_lib, cuda, golden_dir):
    P, hm, _ = _render(golden_dir)
    am, res, X_am, X_cor, _ = _run(P, hm, cuda)
    assert np.array_equal(res.points2d.cpu().numpy(), am.cpu().numpy())
    assert np.array_equal(X_cor.cpu().numpy(), X_am.cpu().numpy())


def test_scenario_planted_distractors_are_corrected(native_lib, cuda, golden_dir):
    from deepfly3d_amd.config import bone_tree

    P, hm_clean, cell = _render(golden_dir)
    T = hm_clean.shape[1]
    am_clean, _, X_clean, _, _ = _run(P, hm_clean, cuda)
    am_clean, X_clean = am_clean.cpu().numpy(), X_clean.cpu().numpy()
    table = po.seeing_table(ORDER)
    parent, bone = bone_tree()
    rng = np.random.default_rng(3)
    hm = hm_clean.copy()
    cnt0, pts0, vals0 = po.heatmap_peaks(hm_clean.reshape(7 * T, 19, 64, 128), 10)
    cnt0, pts0, vals0 = cnt0.reshape(7, T, 19), pts0.reshape(7, T, 19, 10, 2), vals0.reshape(7, T, 19, 10)
    planted = []
    for t in range(T):
        for j in range(38):
            see = table[j]
            for _ in range(50):   # a distractor that every proposal using it gives away by >= tau in some camera
                a = int(rng.integers(len(see)))
                c, src, left = see[a]
                r0, c0 = cell[(c, t, j)]
                rd, cd = int(rng.integers(2, 62)), int(rng.integers(2, 126))
                if (rd - r0) ** 2 + (cd - c0) ** 2 < 20**2:
                    continue
                plane = np.maximum(hm_clean[c, t, src], _gauss(rd, cd, h=1.0 + rng.uniform(0.1, 0.5)))
                cnt, pts, vals = cnt0[:, t : t + 1].copy(), pts0[:, t : t + 1].copy(), vals0[:, t : t + 1].copy()
                pc, pp, pv = po.heatmap_peaks(plane[None, None], 10)
                cnt[c, 0, src], pts[c, 0, src], vals[c, 0, src] = pc[0, 0], pp[0, 0], pv[0, 0]
                assert pc[0, 0] >= 2 and pp[0, 0, 0, 0] == np.float32(rd) * np.float32(1 / 64) and pp[0, 0, 0, 1] == np.float32(cd) * np.float32(1 / 128)
                am1 = po.og.relayout_19_to_38(pts[:, :, :, 0], ORDER)
                props = po.proposals(P, ORDER, am1, cnt, pts, vals, IMAGE_SHAPE, 10, 64, joints=[j])["all"][0][j]
                uses = _uses_distractor(props["index"], a, 0, len(see), 10)   # the distractor is the arg-max: peak 0
                if not _gives_itself_away(P, props["X"][uses], see, cnt[:, 0], pts[:, 0], tau=30.0):
                    continue
                if props["U"][uses].min() - props["U"][~uses].min() < MARGIN_U:
                    continue
                hm[c, t, src] = plane
                planted.append((t, j, c, src))
                break
    for _ in range(3):   # the bones can still favour a distractor over the clean proposal: such joints get their clean map back
        cnt, pts, vals = po.heatmap_peaks(hm.reshape(7 * T, 19, 64, 128), 10)
        cnt, pts, vals = cnt.reshape(7, T, 19), pts.reshape(7, T, 19, 10, 2), vals.reshape(7, T, 19, 10)
        amh = po.og.relayout_19_to_38(pts[:, :, :, 0], ORDER)
        o_pts = po.solve(po.proposals(P, ORDER, amh, cnt, pts, vals, IMAGE_SHAPE, 10, 64)["kept"], ORDER, amh, cnt, pts, parent, bone)[0]
        wrong = {(int(t), int(j)) for _, t, j in np.argwhere((o_pts != am_clean).any(-1))}
        if not wrong:
            break
        for t, j, c, src in planted:
            if (t, j) in wrong:
                hm[c, t, src] = hm_clean[c, t, src]
        planted = [x for x in planted if (x[0], x[1]) not in wrong]
    assert len(planted) > 0.9 * T * 38
    am, res, X_am, X_cor, _ = _run(P, hm, cuda)
    # the arg-max DLT is pulled away on every distracted joint ...
    move = np.linalg.norm(X_am.cpu().numpy() - X_clean, axis=-1)
    assert all(move[t, j] > MOVE_MM for t, j, _, _ in planted), min(move[t, j] for t, j, _, _ in planted)
    # ... the oracle's solve of the planted maps recovers the clean detections (a check of the case itself) ...
    cnt, pts, vals = po.heatmap_peaks(hm.reshape(7 * T, 19, 64, 128), 10)
    cnt, pts, vals = cnt.reshape(7, T, 19), pts.reshape(7, T, 19, 10, 2), vals.reshape(7, T, 19, 10)
    amh = am.cpu().numpy()
    kept = po.proposals(P, ORDER, amh, cnt, pts, vals, IMAGE_SHAPE, 10, 64)["kept"]
    o_pts = po.solve(kept, ORDER, amh, cnt, pts, parent, bone)[0]
    assert np.array_equal(o_pts, am_clean)
    # ... and so does the device, bit for bit, and with it the triangulation
    assert np.array_equal(res.points2d.cpu().numpy(), am_clean)
    assert np.array_equal(X_cor.cpu().numpy(), X_clean)


def _uses_distractor(index, a, slot_d, ns, k):
    """Proposals built on peak `slot_d` of the a-th seeing camera (proposal 0 is the arg-max = the distractor)."""
    uses = index == 0
    pairs = [(0, 1), (0, 2), (1, 2)][: ns * (ns - 1) // 2]
    for q, (pa, pb) in enumerate(pairs):
        sel = (index >= 1 + q * k * k) & (index < 1 + (q + 1) * k * k)
        i, jj = (index - 1 - q * k * k) // k, (index - 1) % k
        if pa == a:
            uses |= sel & (i == slot_d)
        if pb == a:
            uses |= sel & (jj == slot_d)
    return uses


def _gives_itself_away(P, Xs, see, cnt, pts, tau):
    """Every proposal in Xs reprojects >= tau from every peak in at least one seeing camera (or lies behind one)."""
    for X in Xs:
        worst = 0.0
        for c, src, left in see:
            u = P[c] @ np.append(X, 1.0)
            n = int(cnt[c, src])
            if not (u[2] > 0) or n == 0 or not np.all(np.isfinite(u)):
                worst = np.inf
                break
            r = pts[c, src, :n, 0].astype(np.float64) * 480
            cl = pts[c, src, :n, 1].astype(np.float64)
            cl = (1.0 - cl if left else cl) * 960
            worst = max(worst, np.sqrt((u[0] / u[2] - cl) ** 2 + (u[1] / u[2] - r) ** 2).min())
        if worst < tau:
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------ pipeline
def _sample_folder(tmp_path, golden_dir):
    src = os.path.join(golden_dir, "images")
    folder = tmp_path / "working"
    folder.mkdir()
    for f in os.listdir(src):
        os.symlink(os.path.join(src, f), folder / f)
    return str(folder)


def test_inference_folder_returns_peaks(native_lib, cuda, golden_dir, monkeypatch):
    from deepfly3d_amd.inference import inference_folder

    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    folder = os.path.join(golden_dir, "images")
    base = inference_folder(folder, camera_ids_to_flip=[4, 5, 6], max_img_id=1)
    out = inference_folder(folder, camera_ids_to_flip=[4, 5, 6], max_img_id=1, return_peaks=10)
    assert len(out) == 5
    assert np.array_equal(out[0], base[0]) and np.array_equal(out[1], base[1])
    count, pts, vals = out[2:]
    assert count.shape == (7, 2, 19) and pts.shape == (7, 2, 19, 10, 2) and vals.shape == (7, 2, 19, 10)
    assert np.all(count >= 1)
    assert np.array_equal(pts[:, :, :, 0], out[0]) and np.array_equal(vals[:, :, :, 0], out[1][..., 0])
    dev = inference_folder(folder, camera_ids_to_flip=[4, 5, 6], max_img_id=1, return_peaks=10, as_device_tensors=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev)
    assert np.array_equal(dev[3].cpu().numpy(), pts)


def _cli(launcher, folder, env, root, extra=()):
    r = subprocess.run(launcher + [folder, "-n", "2", "-vv", "--auto-correct", *extra], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = [f for f in os.listdir(folder + "_df3d") if f.startswith("df3d_result")]
    assert len(files) == 1
    with open(os.path.join(folder + "_df3d", files[0]), "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("order", [ORDER, [6, 5, 4, 3, 2, 1, 0]], ids=["identity", "rev"])
def test_cli_auto_correct_matches_the_oracle(native_lib, cuda, tmp_path, golden_dir, monkeypatch, order):
    """--order 6 5 4 3 2 1 0 (a rig ordering of core._KNOWN_ORDERINGS) on the sample recording: the flip list pose2d_estimation
    derives from the ordering, the re-layout and auto_correct together."""
    from deepfly3d_amd.config import bone_tree
    from deepfly3d_amd.inference import inference_folder
    from oracle import geometry as og

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DF3D_SYNTHETIC_WEIGHTS="0", PYTHONPATH=root)
    folder = _sample_folder(tmp_path, golden_dir)
    res = _cli([sys.executable, "-m", "deepfly3d_amd.cli"], folder, env, root, extra=("--order", *map(str, order)))
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    keys = list(res.keys())
    assert [str(k) for k in keys] == [str(k) for k in g3["key_order"]] + ["points2d_argmax"]
    assert list(res["camera_ordering"]) == order
    # the oracle's solve on the peaks inference_folder returns, with the cameras the run calibrated
    monkeypatch.setenv("DF3D_SYNTHETIC_WEIGHTS", "0")
    _, _, count, pts, vals = inference_folder(folder, camera_ids_to_flip=[order[i] for i in (4, 5, 6)], max_img_id=1, return_peaks=10)
    P = og.projection_matrices(*(np.stack([res[c][n] for c in range(7)]) for n in ("R", "tvec", "intr")))
    am = res["points2d_argmax"]
    assert np.array_equal(am, og.relayout_19_to_38(pts[:, :, :, 0], order))
    kept = po.proposals(P, order, am, count, pts, vals, IMAGE_SHAPE, 10, 64)["kept"]
    parent, bone = bone_tree()
    o_pts, _, _, margin = po.solve(kept, order, am, count, pts, parent, bone)
    clear = margin > 1e-9   # joints whose optimum beats every other choice by more than 1e-9 (FMA rounding may flip closer ties)
    assert clear.mean() > 0.5
    assert np.array_equal(res["points2d"][:, clear], o_pts[:, clear])


def test_cli_auto_correct_two_ranks_match_one_rank(native_lib, cuda, tmp_path, golden_dir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DF3D_SYNTHETIC_WEIGHTS="0", DF3D_DIST_BACKEND="gloo", PYTHONPATH=root)
    results = []
    for tag, launcher in (("one", [sys.executable, "-m", "deepfly3d_amd.cli"]),
                          ("two", [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                   "--master-port", "29637", "-m", "deepfly3d_amd.cli"])):
        base = tmp_path / tag
        base.mkdir()
        results.append(_cli(launcher, _sample_folder(base, golden_dir), env, root))
    one, two = results
    assert list(one.keys()) == list(two.keys())
    for k in ("points2d", "points2d_argmax", "heatmap_confidence", "camera_ordering"):
        assert np.array_equal(one[k], two[k]), k
    assert np.allclose(one["points3d_wo_procrustes"], two["points3d_wo_procrustes"], atol=1e-9)
