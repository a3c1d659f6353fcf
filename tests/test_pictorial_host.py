"""CPU tests of the pictorial-structures correction: the float64 oracle's exact chain solve against brute
force, the bone tree built from the skeleton constants, the CLI flag, and the argument validation of the new C entries
(no device is touched)."""
import ctypes

import numpy as np
import pytest

import pictorial_oracle as po


def test_oracle_chain_dp_equals_brute_force():
    rng = np.random.default_rng(0)
    for trial in range(60):
        L = 5 if trial % 3 else int(rng.integers(1, 5))
        n = [int(rng.integers(1, 7)) for _ in range(L)]
        U = [rng.normal(0, 1, size=k) for k in n]
        X = [rng.normal(0, 0.6, size=(k, 3)) for k in n]
        mu = [0.0] + list(rng.uniform(0.3, 1.2, size=L - 1))
        sg = [1.0] + list(rng.uniform(0.1, 0.5, size=L - 1))
        wb = float(rng.uniform(0.2, 3.0))
        e, ch = po.chain_dp(U, X, mu, sg, wb)
        eb, chb = po.chain_brute(U, X, mu, sg, wb)
        assert abs(e - eb) <= 1e-12 * max(1.0, abs(eb)), (trial, e, eb)
        assert abs(po.chain_energy(U, X, mu, sg, ch, wb) - eb) <= 1e-12 * max(1.0, abs(eb))
        assert ch == chb, (trial, ch, chb)


def test_bone_tree_is_six_chains_and_eight_single_joints():
    from deepfly3d_amd.config import BONE_MEAN, BONE_STD, TRACKED, bone_tree

    parent, bone = bone_tree()
    chains = po.chains_from_parent(parent)
    lengths = sorted(len(c) for c in chains)
    assert lengths == [1] * 8 + [5] * 6
    assert sum(p >= 0 for p in parent) == 24
    for c in chains:
        if len(c) == 5:
            assert c == list(range(c[0], c[0] + 5)) and TRACKED[c[0]] == 0   # body-coxa roots its leg
    assert np.all(bone[parent >= 0] == (BONE_MEAN, BONE_STD)) and np.all(bone[parent < 0] == 0)
    # the singletons are the antennae and the stripes of both sides
    assert sorted(c[0] for c in chains if len(c) == 1) == [15, 16, 17, 18, 34, 35, 36, 37]


def test_seeing_table_follows_the_relayout():
    t = po.seeing_table([0, 1, 2, 3, 4, 5, 6])
    assert [c for c, _, _ in t[0]] == [0, 1, 2] and [c for c, _, _ in t[15]] == [0, 1]
    assert [c for c, _, _ in t[19]] == [4, 5, 6] and [c for c, _, _ in t[34]] == [5, 6]
    assert all(left for _, _, left in t[20]) and not any(left for _, _, left in t[3])
    assert [s for _, s, _ in t[20]] == [1, 1, 1]


def test_oracle_peak0_is_the_argmax():
    from oracle import geometry as og

    rng = np.random.default_rng(1)
    hm = rng.integers(0, 6, size=(3, 5, 8, 16)).astype(np.float32)   # many ties and plateaus
    count, pts, vals = po.heatmap_peaks(hm, 4)
    am, conf = og.heatmap_argmax(hm)
    assert np.all(count >= 1)
    assert np.array_equal(pts[:, :, 0], am) and np.array_equal(vals[:, :, 0], conf)


def test_cli_auto_correct_flag():
    from deepfly3d_amd.cli import parse_cli_args

    assert parse_cli_args(["/tmp/x", "--auto-correct"]).auto_correct is True
    assert parse_cli_args(["/tmp/x"]).auto_correct is False
    with pytest.raises(SystemExit) as e:
        parse_cli_args(["/tmp/x", "--auto-correct", "--skip-pose-estimation"])
    assert e.value.code == 2


def test_new_entries_validate_arguments_without_gpu(native_lib):
    p16 = ctypes.c_void_p(4096)
    lib = native_lib
    assert lib.df3d_heatmap_peaks(p16, 1, 19, 64, 128, 17, p16, p16, p16, None) == -1 and b"k must be" in lib.df3d_last_error()
    assert lib.df3d_heatmap_peaks(p16, 1, 19, 48, 128, 4, p16, p16, p16, None) == -1 and b"powers of two" in lib.df3d_last_error()
    assert lib.df3d_heatmap_peaks(ctypes.c_void_p(4100), 1, 19, 64, 128, 4, p16, p16, p16, None) == -1 and b"16-byte" in lib.df3d_last_error()
    assert lib.df3d_heatmap_peaks(None, 1, 19, 64, 128, 4, None, None, None, None) == -1 and b"null" in lib.df3d_last_error()
    assert lib.df3d_heatmap_peaks(None, 0, 19, 64, 128, 4, None, None, None, None) == 0   # nothing to do

    P = (ctypes.c_double * 84)(*([1.0] * 84))
    order = (ctypes.c_int * 7)(0, 1, 2, 3, 4, 5, 6)
    bad_order = (ctypes.c_int * 7)(0, 1, 2, 3, 4, 5, 5)

    def prop(order=order, T=4, t0=0, tn=4, k=10, m=64, tau=30.0, P=P):
        return lib.df3d_ps_proposals(P, order, p16, p16, p16, p16, T, t0, tn, k, m, 480.0, 960.0, tau, 1.0, 1.0, p16, p16, p16, p16, p16, None)

    assert prop(bad_order) == -1 and b"permutation" in lib.df3d_last_error()
    assert prop(t0=2, tn=3) == -1 and b"frame range" in lib.df3d_last_error()
    assert prop(k=0) == -1 and prop(m=257) == -1 and prop(tau=0.0) == -1
    assert prop(P=(ctypes.c_double * 84)(*([float("nan")] * 84))) == -1 and b"finite" in lib.df3d_last_error()
    assert prop(tn=0) == 0

    from deepfly3d_amd.config import bone_tree

    parent, bone = bone_tree()
    par = (ctypes.c_int * 38)(*[int(v) for v in parent])
    bn = (ctypes.c_double * 76)(*bone.reshape(-1))

    def solve(par=par, bn=bn, tn=4, work=38 * 4):
        return lib.df3d_ps_solve(order, par, bn, 1.0, p16, p16, p16, 4, 0, tn, 10, 64, p16, p16, p16, p16, p16, p16, p16, p16, p16, work, None)

    assert solve(work=10) == -1 and b"work buffer" in lib.df3d_last_error()
    two_children = list(parent)
    two_children[2] = 0
    assert solve(par=(ctypes.c_int * 38)(*two_children)) == -1 and b"one joint only" in lib.df3d_last_error()
    cycle = list(parent)
    cycle[0] = 4
    every_bone = (ctypes.c_double * 76)(*([0.9, 0.3] * 38))
    assert solve(par=(ctypes.c_int * 38)(*cycle), bn=every_bone) == -1 and b"cycle" in lib.df3d_last_error()
    no_sigma = bone.copy()
    no_sigma[1, 1] = 0.0
    assert solve(bn=(ctypes.c_double * 76)(*no_sigma.reshape(-1))) == -1 and b"deviation" in lib.df3d_last_error()
    assert solve(tn=0) == 0


def test_python_entries_refuse_bad_shapes():
    torch = pytest.importorskip("torch")
    from deepfly3d_amd import ops

    with pytest.raises(ValueError):
        ops.heatmap_peaks(torch.zeros((1, 19, 64, 128)), 4)   # a CPU tensor: the kernels run on the device only
