"""GPU tests of the wavelet spectrogram: csrc/spectrogram.hip against the float64 oracle of
tests/spectrogram_oracle.py.  The bound is derived, not tuned: |device - oracle| <= 16 (2 K_i + 64) 2^-53 max_t |x[:, c]| per element
(so.tolerance), NaN positions identical, the float32 output within one float32 ulp of the rounded oracle.  Every comparison prints
its largest error as a fraction of the bound before it asserts."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrogram_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 320
BANK30 = (30.0, so.frequencies(30.0, 1.0, 7.5, 8))     # K = 144..20
BANK100 = (100.0, so.frequencies(100.0))               # the default: K = 478..20


def _series(T, C, seed=0, scale=1.0):
    rng = np.random.default_rng(1000 * seed + T + C)
    t = np.arange(T)[:, None]
    x = rng.standard_normal((T, C)) + 2.0 * np.sin(2 * np.pi * (1.0 + np.arange(C)[None, :] % 7) * t / 50.0) + 0.5 * np.arange(C)[None, :]
    return np.ascontiguousarray(x * scale)


def _run(cuda, x, fps, freqs, dtype=torch.float64, **kw):
    from deepfly3d_amd import ops

    out = ops.wavelet_spectrogram(torch.from_numpy(np.ascontiguousarray(x)).to(cuda), fps, freqs, dtype=dtype, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, x, fps, freqs, what, omega0=so.OMEGA0, radius=so.RADIUS, want=None):
    """The device result against the oracle under the derived bound; returns the oracle's result."""
    want = so.spectrogram(x, fps, freqs, omega0, radius) if want is None else want
    assert got.shape == want.shape and got.dtype == np.float64, what
    flat = (x.shape[0], int(np.prod(x.shape[1:])), len(freqs))
    g, w = got.reshape(flat), want.reshape(flat)
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: NaN positions differ"
    assert not np.isinf(g).any(), what
    tol = so.tolerance(x, fps, freqs, omega0, radius)[None]
    err = np.where(np.isnan(w), 0.0, np.abs(g - w))
    with np.errstate(all="ignore"):
        frac = np.where(err > 0, err / tol, 0.0).max() if err.size else 0.0
    print(f"{what}: max |device - oracle| = {err.max() if err.size else 0.0:.3g}, {frac:.3g} of the bound")
    assert np.all(err <= tol), what
    return want


# ------------------------------------------------------------------------------------------------------------------ sizes
def test_tile_constant(native_lib):
    from deepfly3d_amd import config as cfg

    assert native_lib.df3d_spectrogram_tile() == cfg.SPECTROGRAM_TILE == TILE


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_lengths_around_the_wave_and_the_tile(native_lib, cuda, T):
    x = _series(T, 3)
    _check(_run(cuda, x, *BANK30), x, *BANK30, f"T = {T}")


@pytest.mark.parametrize("T", [700, 1300])
def test_default_bank(native_lib, cuda, T):
    """T = 700 is shorter than 2 K_0 = 956: every time of row 0 leans on an edge; 1300 has an interior.  Both span several tiles."""
    x = _series(T, 3, seed=1)
    want = _check(_run(cuda, x, *BANK100), x, *BANK100, f"default bank, T = {T}")
    got32 = _run(cuda, x, *BANK100, dtype=torch.float32)
    assert got32.dtype == np.float32 and got32.shape == want.shape
    w32 = want.astype(np.float32)
    assert np.all(np.abs(got32 - w32) <= np.spacing(np.abs(w32)))          # at most one float32 ulp from the rounded oracle
    assert np.array_equal(got32, _run(cuda, x, *BANK100).astype(np.float32))   # and the float64 result rounded once, exactly


@pytest.mark.parametrize("C", [1, 3, 48])
def test_channel_counts(native_lib, cuda, C):
    x = _series(TILE + 81, C, seed=2)
    _check(_run(cuda, x, *BANK30), x, *BANK30, f"C = {C}")


@pytest.mark.parametrize("F", [1, 25, 64])
def test_row_counts(native_lib, cuda, F):
    """1 row, 25 rows (two chunks of the kernel's 16, the second one partial) and the most, 64."""
    fps = 100.0
    freqs = so.frequencies(fps, 2.0, 50.0, F) if F > 1 else np.array([3.0])
    x = _series(401, 2, seed=3)
    got = _run(cuda, x, fps, freqs)
    _check(got, x, fps, freqs, f"F = {F}")
    got32 = _run(cuda, x, fps, freqs, dtype=torch.float32)
    assert np.array_equal(got32, got.astype(np.float32))


def test_support_at_the_cap_and_other_wavelets(native_lib, cuda):
    from deepfly3d_amd import config as cfg
    from deepfly3d_amd import ops

    fps = 100.0
    f0 = 6.0 * 5.0 * fps / (2.0 * np.pi * cfg.SPECTROGRAM_MAX_SUPPORT) * (1 + 1e-12)
    freqs = np.array([f0, 10.0])
    assert list(ops.wavelet_support(fps, freqs)) == [2048, 48]
    x = _series(700, 1, seed=4)
    _check(_run(cuda, x, fps, freqs), x, fps, freqs, "K_0 = 2048")
    with pytest.raises(ValueError, match="cap of 2048"):
        ops.wavelet_spectrogram(torch.from_numpy(x).to(cuda), fps, np.array([f0 * 0.999, 10.0]))
    x = _series(500, 2, seed=5)
    for omega0, radius in ((6.0, 4.0), (3.0, 7.5)):
        _check(_run(cuda, x, *BANK30, omega0=omega0, radius=radius), x, *BANK30, f"omega0 = {omega0}, radius = {radius}", omega0, radius)
    # unsorted rows are refused, repeated ones are not
    twice = np.array([2.0, 2.0, 5.0])
    got = _run(cuda, x, 30.0, twice)
    _check(got, x, 30.0, twice, "a repeated row")
    assert np.array_equal(got[..., 0], got[..., 1])


# ------------------------------------------------------------------------------------------------------------------ values
def test_non_finite_samples(native_lib, cuda):
    T = 2 * TILE + 60
    base = _series(T, 4, seed=6)
    K = so.support(*BANK30)
    cases = {"first": [(0, 1, np.nan)], "last": [(T - 1, 2, np.inf)], "tile boundary": [(TILE - 1, 0, -np.inf), (TILE, 3, np.nan)],
             "one per channel": [(17, 0, np.nan), (TILE + 3, 1, np.inf), (400, 2, -np.inf), (T - 2, 3, np.nan)],
             "a whole channel": [(t, 1, np.nan) for t in range(T)]}
    clean = _run(cuda, base, *BANK30)
    for name, marks in cases.items():
        x = base.copy()
        for t0, c, v in marks:
            x[t0, c] = v
        got = _run(cuda, x, *BANK30)
        _check(got, x, *BANK30, f"non-finite, {name}")
        touched = sorted({c for _, c, _ in marks})
        others = [c for c in range(4) if c not in touched]
        assert got[:, others].tobytes() == clean[:, others].tobytes(), name     # every other channel bit-equal
        if len(marks) < T:
            for t0, c, _ in marks:
                if 0 < t0 < T - 1:
                    for i, k in enumerate(K):
                        nan = np.flatnonzero(np.isnan(got[:, c, i]))
                        assert nan[0] == max(0, t0 - k) and nan[-1] == min(T - 1, t0 + k) and len(nan) == nan[-1] - nan[0] + 1, (name, t0, i)
        assert np.array_equal(np.isnan(_run(cuda, x, *BANK30, dtype=torch.float32)), np.isnan(got)), name


@pytest.mark.parametrize("scale", [1e-6, 1e6])
def test_scaled_inputs(native_lib, cuda, scale):
    x = _series(TILE + 130, 3, seed=7, scale=scale)
    _check(_run(cuda, x, *BANK30), x, *BANK30, f"scale {scale:g}")


def test_constant_and_sinusoid(native_lib, cuda):
    fps, freqs = BANK100
    T = 1000
    x = np.empty((T, 2))
    x[:, 0] = -7.5
    x[:, 1] = 0.7 * np.sin(2 * np.pi * freqs[12] * np.arange(T) / fps)
    got = _run(cuda, x, fps, freqs)
    assert np.abs(got[:, 0]).max() <= 1e-12 * 7.5
    K12 = int(so.support(fps, freqs)[12])
    inner = got[K12 + 1 : T - K12 - 1, 1]
    assert np.abs(inner[:, 12] / 0.7 - 1.0).max() <= 1e-6 and np.all(np.argmax(inner, axis=1) == 12)


# ------------------------------------------------------------------------------------------------------------------ the C entries
def test_guard_words_sentinels_and_a_side_stream(native_lib, cuda):
    """The raw entries on buffers filled with a sentinel, guard words on both sides of the output and of the workspace, on a stream of
    its own: every output element is written, nothing outside is, and the bank stays inside the bytes the size query names."""
    lib = native_lib
    fps, freqs = BANK30
    T, C, F, G = TILE + 7, 3, len(freqs), 64
    x = _series(T, C, seed=8)
    fp = freqs.ctypes.data_as(ctypes.c_void_p)
    need = lib.df3d_spectrogram_work_bytes(fp, F, fps, so.OMEGA0, so.RADIUS)
    assert need % 16 == 0 and need >= int(np.sum(2 * so.support(fps, freqs) + 1)) * 16
    sentinel = -1.2345e30   # representable in float32 too
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        xc = torch.from_numpy(x).to(cuda).t().contiguous()
        work = torch.full((need // 8 + 2 * G,), sentinel, dtype=torch.float64, device=cuda)
        for f32 in (0, 1):
            out = torch.full((T * C * F + 2 * G,), sentinel, dtype=torch.float32 if f32 else torch.float64, device=cuda)
            wptr, optr = work.data_ptr() + 8 * G, out.data_ptr() + out.element_size() * G
            assert lib.df3d_spectrogram_bank(fp, F, fps, so.OMEGA0, so.RADIUS, wptr, need, side.cuda_stream) == 0, lib.df3d_last_error()
            assert lib.df3d_spectrogram(xc.data_ptr(), T, C, fp, F, fps, so.OMEGA0, so.RADIUS, wptr, need, optr, f32, side.cuda_stream) == 0, \
                lib.df3d_last_error()
            side.synchronize()
            o, w = out.cpu().numpy(), work.cpu().numpy()
            guard = np.float32(sentinel) if f32 else sentinel
            assert np.all(o[:G] == guard) and np.all(o[-G:] == guard) and not np.any(o[G:-G] == guard)
            assert np.all(w[:G] == sentinel) and np.all(w[-G:] == sentinel)
            got = o[G:-G].reshape(T, C, F)
            if f32:
                assert np.array_equal(got, want64.astype(np.float32))
            else:
                want64 = got.copy()
                _check(got, x, fps, freqs, "raw entries, side stream")
        # the taps the bank kernel wrote are the oracle's, to a few ulp of the largest tap (the sums' order differs)
        pairs = w[G:-G].reshape(-1, 2)
        at = 0
        for f in freqs:
            K, a, b = so.taps(fps, f)
            n = 2 * K + 1
            assert np.abs(pairs[at : at + n, 0] - a).max() <= 40 * 2.0 ** -53 * np.abs(a).max()
            assert np.abs(pairs[at : at + n, 1] - b).max() <= 40 * 2.0 ** -53 * np.abs(a).max()
            at += n
    # through ops on the side stream as well
    from deepfly3d_amd import ops

    with torch.cuda.stream(side):
        got = ops.wavelet_spectrogram(torch.from_numpy(x).to(cuda), fps, freqs)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want64)


def test_shapes_through_ops(native_lib, cuda):
    from deepfly3d_amd import ops

    x = _series(200, 48, seed=9)
    flat = _run(cuda, x, *BANK30)
    assert np.array_equal(_run(cuda, x.reshape(200, 6, 8), *BANK30), flat.reshape(200, 6, 8, 8))
    assert np.array_equal(_run(cuda, x[:, 5].copy(), *BANK30), flat[:, 5])
    _check(flat.reshape(200, 6, 8, 8), x.reshape(200, 6, 8), *BANK30, "[T, 6, 8]")
    view = torch.from_numpy(x).to(cuda)[:, ::2]   # not contiguous: ops copies
    assert np.array_equal(ops.wavelet_spectrogram(view, *BANK30).cpu().numpy(), flat[:, ::2])
    empty = ops.wavelet_spectrogram(torch.zeros((0, 6, 8), dtype=torch.float64, device=cuda), *BANK30)
    assert empty.shape == (0, 6, 8, 8) and empty.dtype == torch.float64
    with pytest.raises(ValueError, match="at least one channel"):
        ops.wavelet_spectrogram(torch.zeros((5, 0), dtype=torch.float64, device=cuda), *BANK30)
    with pytest.raises(ValueError, match="series"):
        ops.wavelet_spectrogram(torch.zeros((5, 2), dtype=torch.float32, device=cuda), *BANK30)
    # the default bank is wavelet_frequencies(fps)
    d = ops.wavelet_spectrogram(torch.from_numpy(x[:, :1].copy()).to(cuda), 100.0)
    assert d.shape == (200, 1, 25)


# ------------------------------------------------------------------------------------------------------------------ Core and the CLI
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


SPECTRO_KEYS = ["angle_spectrogram", "spectrogram_freqs", "spectrogram_fps"]
RIGID_KEYS = ["points3d_rigid", "rigid_segment_lengths", "rigid_fit_cost"]


def _unwrapped(angles):
    from deepfly3d_amd import config as cfg

    series = angles.reshape(angles.shape[0], 48).copy()
    cols = [8 * leg + cfg.LEG_ANGLE_NAMES.index(a) for leg in range(6) for a in cfg.SPECTROGRAM_UNWRAPPED_ANGLES]
    series[:, cols] = np.unwrap(series[:, cols], axis=0)
    return series, cols


def test_core_angle_spectrogram(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import ops
    from deepfly3d_amd.config import config
    from deepfly3d_amd.core import Core

    config.pop("image_shape", None)
    folder, pkl = _recording(tmp_path, golden_dir)
    core = Core(folder, folder + "_df3d", num_images_max=0, camera_ordering=list(range(7)))
    assert core.get_fps() is None
    S, freqs = core.angle_spectrogram()   # triangulates first; no videos: 100 fps
    assert S.shape == (15, 6, 8, 25) and S.dtype == np.float64 and np.array_equal(freqs, so.frequencies(100.0))
    for rigid in (False, True):
        S, freqs = core.angle_spectrogram(rigid=rigid)
        series, cols = _unwrapped(core.joint_angles(rigid=rigid)[0])
        dev = ops.unwrap_phase(torch.from_numpy(core.joint_angles(rigid=rigid)[0].reshape(15, 48)).to(cuda), cols)[0].cpu().numpy()
        assert np.abs(dev - series).max() <= 1e-12
        _check(S, dev.reshape(15, 6, 8), 100.0, freqs, f"Core.angle_spectrogram(rigid={rigid})")
    # the bank's arguments, another frame rate, no unwrapping
    S30, f30 = core.angle_spectrogram(fps=30.0, f_max=7.5, num=8, unwrap=False)
    assert np.array_equal(f30, BANK30[1])
    _check(S30, core.joint_angles()[0], 30.0, f30, "Core.angle_spectrogram(fps=30, unwrap=False)")
    Sf, ff = core.angle_spectrogram(freqs=[2.0, 4.0], omega0=6.0)
    _check(Sf, _unwrapped(core.joint_angles()[0])[0].reshape(15, 6, 8), 100.0, ff, "Core.angle_spectrogram(freqs=...)", omega0=6.0)
    # save: the new keys after every existing one, float32
    core.save(joint_angles=True, rigid_legs=True)
    before = _load(pkl)
    core.save(joint_angles=True, rigid_legs=True, angle_spectrogram=True)
    flagged = _load(pkl)
    assert list(flagged.keys()) == list(before.keys()) + SPECTRO_KEYS + ["angle_spectrogram_rigid"]
    assert all(_same(before[k], flagged[k]) for k in before)
    assert flagged["angle_spectrogram"].dtype == np.float32 and flagged["angle_spectrogram"].shape == (15, 6, 8, 25)
    assert np.array_equal(flagged["angle_spectrogram"], core.angle_spectrogram()[0].astype(np.float32))
    assert np.array_equal(flagged["angle_spectrogram_rigid"], core.angle_spectrogram(rigid=True)[0].astype(np.float32))
    assert np.array_equal(flagged["spectrogram_freqs"], so.frequencies(100.0)) and flagged["spectrogram_fps"] == 100.0
    core.save(angle_spectrogram=True)
    assert list(_load(pkl).keys()) == [k for k in before.keys() if k not in RIGID_KEYS + ["joint_angles", "segment_lengths", "joint_angles_rigid"]] + SPECTRO_KEYS
    config.pop("image_shape", None)


def test_cli_skip_pose_estimation_angle_spectrogram_rigid_legs(native_lib, cuda, tmp_path, golden_dir):
    from deepfly3d_amd import cli, ops
    from deepfly3d_amd.config import config

    config.pop("image_shape", None)
    g3 = np.load(f"{golden_dir}/golden_3d.npz")
    folder, pkl = _recording(tmp_path, golden_dir)
    with open(pkl, "rb") as f:
        earlier = f.read()
    order = [str(c) for c in range(7)]

    def reopen(*flags):
        with open(pkl, "wb") as f:
            f.write(earlier)
        assert cli.main([folder, "--skip-pose-estimation", *flags, "--order"] + order) == 0
        return _load(pkl)

    plain = reopen("--rigid-legs")
    run = reopen("--angle-spectrogram", "--rigid-legs")
    assert [str(k) for k in run.keys()] == [str(k) for k in g3["key_order"]] + RIGID_KEYS + SPECTRO_KEYS + ["angle_spectrogram_rigid"]
    assert all(_same(plain[k], run[k]) for k in plain)   # no joint_angles key: the flag computes the angles itself and does not store them
    for key, pose in (("angle_spectrogram", run["points3d_wo_procrustes"]), ("angle_spectrogram_rigid", run["points3d_rigid"])):
        assert run[key].shape == (15, 6, 8, 25) and run[key].dtype == np.float32
        X = torch.from_numpy(np.ascontiguousarray(run["points3d_wo_procrustes"])).to(cuda)
        frame = ops.recording_frame(X)
        angles = ops.joint_angles(torch.from_numpy(np.ascontiguousarray(pose)).to(cuda), frame)[0].cpu().numpy()
        series, _ = _unwrapped(angles)
        want = so.spectrogram(series.reshape(15, 6, 8), 100.0, run["spectrogram_freqs"])
        tol = so.tolerance(series, 100.0, run["spectrogram_freqs"]).reshape(1, 6, 8, 25)
        err = np.abs(run[key].astype(np.float64) - want)
        print(f"{key}: {np.max(err / (tol + np.spacing(want.astype(np.float32)))):.3g} of the bound plus one float32 ulp")
        assert np.all(err <= tol + np.spacing(want.astype(np.float32)))
    assert np.array_equal(run["spectrogram_freqs"], so.frequencies(100.0)) and run["spectrogram_fps"] == 100.0
    only = reopen("--angle-spectrogram", "--joint-angles")
    assert [str(k) for k in only.keys()] == [str(k) for k in g3["key_order"]] + ["joint_angles", "segment_lengths"] + SPECTRO_KEYS
    assert _same(only["angle_spectrogram"], run["angle_spectrogram"])
    config.pop("image_shape", None)
