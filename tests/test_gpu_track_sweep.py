"""-m gpu sweep of the tracking of the 2-D detections (csrc/track.hip, DESIGN.md section 22, "swept"): the families of tests/track_cases.py
on the device, choice and cost equal to the int64 oracle exactly.  tests/test_track_cases_host.py certifies on the CPU that each family
does what it is here for; nothing is skipped or relaxed at run time."""
import numpy as np
import pytest
import torch

import track_cases as tc
import track_oracle as to
from oracle import geometry as og

pytestmark = pytest.mark.gpu

IMAGE_SHAPE = [960, 480]   # [W, H], as Core carries it


def _device(arrays, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _check(ops, dev, want, image_hw, params, block, label):
    C, T, J = want[0].shape
    tau, wm, wv = params
    r = ops.track_peaks(*dev, [image_hw[1], image_hw[0]], tau=tau, w_motion=wm, w_value=wv, block_frames=block)
    choice, cost = r.choice.cpu().numpy(), r.cost.cpu().numpy()
    assert choice.dtype == np.int32 and cost.dtype == np.int64 and choice.shape == (C, T, J) and cost.shape == (C, J), label
    assert np.array_equal(cost, want[1]), label
    assert np.array_equal(choice, want[0]), label


DEFAULTS = (to.TAU, to.W_MOTION, to.W_VALUE)


@pytest.mark.parametrize("C,J", tc.MANY_CHAINS, ids=[f"{C * J} chains" for C, J in tc.MANY_CHAINS])
def test_many_chains(native_lib, cuda, C, J):
    """15, 16, 17, 255, 256, 257 and 513 chains: the carry kernel's 16 chains per workgroup and the exit kernel's 256 at, below and above
    their edges; with T = 37 and block 5 every chain has eight blocks, and chain nb + b is taken past chain 256.  The costs of a launch
    are pairwise distinct (certified), so chains that are permuted or doubled change the answer."""
    from deepfly3d_amd import ops

    for T in tc.MANY_T:
        peaks = tc.many_chains(C, J, T)
        want, dev = to.solve(*peaks, tc.IMAGE_HW), _device(peaks, cuda)
        for block in tc.MANY_BLOCKS:
            _check(ops, dev, want, tc.IMAGE_HW, DEFAULTS, block, (C, J, T, block))


@pytest.mark.parametrize("K", tc.HALFWAY_K)
def test_halfway_costs_round_to_even(native_lib, cuda, K):
    """Costs that are x.5 before rint, exactly: half of the pair costs and a third or more of the unary ones (certified)."""
    from deepfly3d_amd import ops

    peaks = tc.halfway(600 + K, K)
    want, dev = to.solve(*peaks, tc.HALFWAY_HW, *tc.HALFWAY_PARAMS), _device(peaks, cuda)
    for block in (16, 256):
        _check(ops, dev, want, tc.HALFWAY_HW, tc.HALFWAY_PARAMS, block, (K, block))


@pytest.mark.parametrize("params", tc.WEIGHTS, ids=[f"tau {t:g} w_m {m:g} w_v {v:g}" for t, m, v in tc.WEIGHTS])
def test_weights_and_tau_at_their_ends(native_lib, cuda, params):
    """The largest weights (2^30 in the int pair table, chain costs beyond 2^31), a weight of 0, a tau below and above every jump, and
    weights that quantise to 0 (the tie rule alone decides) and to 2."""
    from deepfly3d_amd import ops

    for T in tc.WEIGHTS_T:
        peaks = tc.weights_case(T)
        want, dev = to.solve(*peaks, tc.IMAGE_HW, *params), _device(peaks, cuda)
        for block in (5, 256):
            _check(ops, dev, want, tc.IMAGE_HW, params, block, (params, T, block))


@pytest.mark.parametrize("B", tc.SWEEP_BLOCKS)
def test_placeholders_by_design(native_lib, cuda, B):
    """One chain per pattern of track_cases.PLACEHOLDER_PATTERNS: all frames, the first, the last, both sides of every block edge, a whole
    chunk, a whole ring, every other frame, a valid frame between two runs."""
    from deepfly3d_amd import ops

    peaks = tc.placeholders(50 + B, B)
    want = to.solve(*peaks, tc.IMAGE_HW)
    _check(ops, _device(peaks, cuda), want, tc.IMAGE_HW, DEFAULTS, B, B)
    assert not want[0][0][tc.placeholder_frames(B).T].any()


@pytest.mark.parametrize("B", tc.SWEEP_BLOCKS)
def test_designed_ties(native_lib, cuda, B):
    """Every path costs 0: slot 0 throughout, and slot 1 in exactly the frames whose slot 0 is invalid -- a block's first frame, a block's
    last frame and the last frame among them."""
    from deepfly3d_amd import ops

    count, pts, val, wanted = tc.designed_ties(B)
    want = to.solve(count, pts, val, tc.IMAGE_HW)
    assert np.array_equal(want[0], wanted) and not want[1].any()
    _check(ops, _device((count, pts, val), cuda), want, tc.IMAGE_HW, DEFAULTS, B, B)


@pytest.mark.parametrize("K", tc.ODD_K)
def test_blocks_that_are_not_whole_chunks(native_lib, cuda, K):
    """Blocks of 15 to 513 frames, none a multiple of the 16-frame chunk, with recordings one frame short of a block, a block, a block
    and a frame, and two blocks and a frame."""
    from deepfly3d_amd import ops

    solved = {}
    for B in tc.ODD_BLOCKS:
        for T in tc.odd_block_times(B):
            if T not in solved:
                peaks = tc.odd_blocks_case(K, T)
                solved[T] = (to.solve(*peaks, tc.IMAGE_HW), _device(peaks, cuda))
            want, dev = solved[T]
            _check(ops, dev, want, tc.IMAGE_HW, DEFAULTS, B, (K, B, T))
    assert max(solved) == 1027


def test_more_than_65535_workgroups(native_lib, cuda):
    """513 chains of 130 frames in blocks of one frame: 66 690 workgroups of the block and trace kernels, and a workspace of
    147 320 448 bytes (df3d_track_work_bytes(513, 130, 2, 1))."""
    from deepfly3d_amd import ops

    w = tc.WIDE_GRID
    assert w["C"] * w["J"] * w["T"] == 66690 > 65535
    assert native_lib.df3d_track_work_bytes(w["C"] * w["J"], w["T"], w["K"], w["block_frames"]) == tc.WIDE_GRID_WORK_BYTES == 147_320_448
    peaks = tc.wide_grid()
    _check(ops, _device(peaks, cuda), to.solve(*peaks, tc.IMAGE_HW), tc.IMAGE_HW, DEFAULTS, w["block_frames"], "wide grid")


def test_guard_words_and_a_dirty_workspace(native_lib, cuda):
    """The C entry on a stream of its own, 513 chains of 37 frames in blocks of 5: choice and cost sentinel-filled inside guard words, the
    workspace exactly df3d_track_work_bytes long inside guard words and pre-filled with 0x00 twice and with 0xFF twice.  Every element of
    choice and cost is written, no guard word is, and the four runs have the same bits, the oracle's: a kernel that read a workspace byte
    no kernel of the same call had written would differ between the fills."""
    lib = native_lib
    C, J = tc.MANY_CHAINS[-1]
    T, K, block, GUARD = 37, tc.MANY_K, 5, 64
    peaks = tc.many_chains(C, J, T)
    want_choice, want_cost = to.solve(*peaks, tc.IMAGE_HW)
    need = lib.df3d_track_work_bytes(C * J, T, K, block)
    assert need > 0 and need % 64 == 0
    side = torch.cuda.Stream(device=cuda)
    fills = {torch.int32: -77, torch.int64: -7777, torch.uint8: 0x5A}

    def guarded(n, dtype, inside=None):
        t = torch.full((n + 2 * GUARD,), fills[dtype], dtype=dtype, device=cuda)
        if inside is not None:
            t[GUARD:GUARD + n] = inside
        return t, t.data_ptr() + GUARD * t.element_size()

    def inner(t):
        a = t.cpu().numpy()
        assert np.all(a[:GUARD] == fills[t.dtype]) and np.all(a[-GUARD:] == fills[t.dtype]), "a guard word was written"
        return a[GUARD:-GUARD]

    runs = []
    with torch.cuda.stream(side):
        count, pts, val = _device(peaks, cuda)
        for fill in (0x00, 0x00, 0xFF, 0xFF):
            choice, cost, work = guarded(C * T * J, torch.int32), guarded(C * J, torch.int64), guarded(need, torch.uint8, fill)
            assert work[1] % 16 == 0
            rc = lib.df3d_track_peaks(count.data_ptr(), pts.data_ptr(), val.data_ptr(), C, T, J, K, float(tc.IMAGE_HW[0]), float(tc.IMAGE_HW[1]),
                                      to.TAU, to.W_MOTION, to.W_VALUE, block, choice[1], cost[1], work[1], need, side.cuda_stream)
            assert rc == 0, lib.df3d_last_error()
            side.synchronize()
            inner(work[0])
            runs.append((inner(choice[0]).copy(), inner(cost[0]).copy()))
    for choice, cost in runs:
        assert not np.any(choice == fills[torch.int32]) and not np.any(cost == fills[torch.int64]), "an output element was not written"
        assert choice.tobytes() == runs[0][0].tobytes() and cost.tobytes() == runs[0][1].tobytes()
    assert np.array_equal(runs[0][0].reshape(C, T, J), want_choice) and np.array_equal(runs[0][1].reshape(C, J), want_cost)


@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0]], ids=["identity", "rev"])
def test_tracked_points2d_at_its_edges(native_lib, cuda, order, K):
    """No frames, a choice that is non-zero everywhere and one that is 0 everywhere, against the numpy re-layout."""
    from deepfly3d_amd import ops

    T = 5
    rng = np.random.default_rng(40 + K)
    pts = rng.random((7, T, 19, K, 2), dtype=np.float32)
    d_pts = torch.from_numpy(pts).to(cuda)
    points2d = ops.relayout_19_to_38(d_pts[:, :, :, 0].contiguous(), order)
    base = points2d.cpu().numpy()
    # T = 0
    empty = ops.tracked_points2d(points2d[:, :0].contiguous(), order, d_pts[:, :0].contiguous(), torch.zeros((7, 0, 19), dtype=torch.int32, device=cuda))
    assert tuple(empty.shape) == (7, 0, 38, 2) and empty.dtype == torch.float64
    # 0 everywhere: the input's bits, whatever they are
    zero = torch.zeros((7, T, 19), dtype=torch.int32, device=cuda)
    marked = torch.full_like(points2d, -7.25)
    assert torch.equal(ops.tracked_points2d(points2d, order, d_pts, zero), points2d)
    assert torch.equal(ops.tracked_points2d(marked, order, d_pts, zero), marked)
    # non-zero everywhere (K = 1 has slot 0 alone: a non-zero choice names no slot and the gather clamps it to the last one)
    choice = rng.integers(1, max(K, 2), size=(7, T, 19)).astype(np.int32)
    out = ops.tracked_points2d(marked, order, d_pts, torch.from_numpy(choice).to(cuda)).cpu().numpy()
    chosen = np.take_along_axis(pts, np.minimum(choice, K - 1)[..., None, None].astype(np.int64), axis=3)[:, :, :, 0]
    moved = og.relayout_19_to_38(np.ones((7, T, 19, 2), np.float32), order)[..., 0] != 0
    assert out.dtype == np.float64 and out.shape == base.shape and moved.any() and not moved.all()
    assert np.array_equal(out[moved], og.relayout_19_to_38(chosen, order)[moved]) and np.all(out[~moved] == -7.25)
