"""CPU tests of the wavelet spectrogram: the float64 oracle's own properties and its independent witness, the C
entries' refusals (no device is touched), ops' argument errors, the unwrap rule, the command-line flag and Core's refusals."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrogram_oracle as so  # noqa: E402


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(16).standard_normal((1300, 3))


# ------------------------------------------------------------------------------------------------------------------ the bank
def test_default_banks():
    f = so.frequencies(100.0)
    K = so.support(100.0, f)
    assert f.shape == (25,) and f[0] == 1.0 and f[-1] == 25.0 and np.all(np.diff(f) > 0)
    assert K[0] == 478 and K[1] == 418 and K[-1] == 20 and int(np.sum(2 * K + 1)) == 7391
    f30 = so.frequencies(30.0, 1.0, 7.5, 8)
    K30 = so.support(30.0, f30)
    assert K30[0] == 144 and K30[-1] == 20
    assert np.array_equal(so.frequencies(100.0, 3.0, 40.0, 1), [3.0])
    for fps, freqs in ((100.0, f), (30.0, f30)):
        for fi in freqs:
            K_, a, b = so.taps(fps, fi)
            assert abs(a.sum()) <= 1e-15 and abs(b.sum()) <= 1e-15   # a constant extension contributes nothing
            assert np.array_equal(a, a[::-1]) and np.array_equal(b, -b[::-1])


def test_unit_sinusoid_reads_its_amplitude_on_its_row():
    fps = 100.0
    freqs = so.frequencies(fps)
    K0 = int(so.support(fps, freqs)[0])
    T = 2 * K0 + 41
    t = np.arange(T)
    inner = slice(K0 + 1, T - K0 - 1)
    worst = 0.0
    for i, f in enumerate(freqs):
        S = so.spectrogram(0.7 * np.sin(2 * np.pi * f * t / fps + 0.3), fps, freqs)[inner]
        worst = max(worst, np.abs(S[:, i] / 0.7 - 1.0).max())
        assert np.all(np.argmax(S, axis=1) == i), i
    print(f"unit sinusoid: worst relative error {worst:.3g}")
    assert worst <= 1e-6


def test_admissibility_term_removes_the_constant_offset():
    fps, T = 100.0, 64
    freqs = so.frequencies(fps)
    x = np.full((T, 1), 3.25)
    S = so.spectrogram(x, fps, freqs)
    assert np.abs(S).max() <= 1e-12 * 3.25
    leak = so.spectrogram(x, fps, freqs, admissible=False) / 3.25
    assert np.allclose(leak, 2.0 * np.exp(-so.OMEGA0 ** 2 / 2.0), rtol=1e-3)   # 7.5e-6 per unit without kappa


def test_image_frequency_folds_in_above_a_quarter_of_the_sampling_rate():
    fps, T = 100.0, 400
    t = np.arange(T)
    for frac, lo, hi in ((0.36, 1e-4, 3e-3), (0.42, 0.05, 0.5), (0.5, 0.9, 1.1)):
        f = frac * fps
        S = so.spectrogram(np.cos(2 * np.pi * f * t / fps), fps, [f])[100:300, 0]
        ripple = (S.max() - S.min()) / 2.0 if frac < 0.5 else S.max() - 1.0   # at Nyquist the image doubles the reading
        assert lo <= ripple <= hi, (frac, ripple)


def test_oracle_agrees_with_the_fft_witness(noise):
    fps = 100.0
    freqs = so.frequencies(fps)
    err = np.abs(so.spectrogram(noise, fps, freqs) - so.witness(noise, fps, freqs)).max()
    print(f"oracle against fftconvolve: {err:.3g}")
    assert err <= 1e-12 * np.abs(noise).max()
    f30 = so.frequencies(30.0, 1.0, 7.5, 8)
    assert np.abs(so.spectrogram(noise[:200], 30.0, f30) - so.witness(noise[:200], 30.0, f30)).max() <= 1e-12 * np.abs(noise).max()


def test_linearity_shift_and_short_series(noise):
    fps = 30.0
    freqs = so.frequencies(fps, 1.0, 7.5, 8)
    K0 = int(so.support(fps, freqs)[0])
    x = noise[:700]
    S = so.spectrogram(x, fps, freqs)
    assert np.array_equal(so.spectrogram(4.0 * x, fps, freqs), 4.0 * S)   # a power of two: exact
    assert np.array_equal(so.spectrogram(-x, fps, freqs), S)
    # a shift by 7 samples moves an interior stretch with it
    y = np.roll(x, 7, axis=0)
    inner = slice(K0 + 8, 700 - K0 - 8)
    assert np.abs(so.spectrogram(y, fps, freqs)[K0 + 15 : 700 - K0 - 1] - S[inner]).max() <= 1e-12
    # T = 1 and T = 2: everything is edge extension
    assert np.abs(so.spectrogram(x[:1], fps, freqs)).max() <= 1e-12 * np.abs(x[:1]).max()
    two = so.spectrogram(x[:2], fps, freqs)
    assert two.shape == (2, 3, 8) and np.all(np.isfinite(two))
    assert np.abs(two - so.witness(x[:2], fps, freqs)).max() <= 1e-12 * np.abs(x[:2]).max()
    assert so.spectrogram(x[:0], fps, freqs).shape == (0, 3, 8)
    assert so.spectrogram(x[:, 0], fps, freqs).shape == (700, 8) and so.spectrogram(x.reshape(700, 3, 1), fps, freqs).shape == (700, 3, 1, 8)


def test_non_finite_samples_spread_over_exactly_their_support(noise):
    fps = 30.0
    freqs = so.frequencies(fps, 1.0, 7.5, 8)
    K = so.support(fps, freqs)
    x = noise[:500].copy()
    S = so.spectrogram(x, fps, freqs)
    for value, t0, c in ((np.nan, 250, 1), (np.inf, 100, 0), (-np.inf, 0, 2), (np.nan, 499, 0)):
        y = x.copy()
        y[t0, c] = value
        R = so.spectrogram(y, fps, freqs)
        for i, k in enumerate(K):
            want = np.zeros(500, dtype=bool)
            want[max(0, t0 - k) : t0 + k + 1] = True
            if t0 == 0 or t0 == 499:   # an edge sample also stands in for everything beyond it: the clamped range
                want[:k + 1] |= t0 == 0
                want[499 - k:] |= t0 == 499
            assert np.array_equal(np.isnan(R[:, c, i]), want), (value, t0, i)
        others = [ch for ch in range(3) if ch != c]
        assert R[:, others].tobytes() == S[:, others].tobytes()
        assert not np.isinf(R).any()


# ------------------------------------------------------------------------------------------------------------------ the C entries
def test_entries_validate_arguments_without_gpu(native_lib):
    from deepfly3d_amd import config as cfg

    lib, err = native_lib, native_lib.df3d_last_error
    assert lib.df3d_spectrogram_tile() == cfg.SPECTROGRAM_TILE
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    freqs = so.frequencies(100.0)
    need = lib.df3d_spectrogram_work_bytes(ptr(freqs), 25, 100.0, 5.0, 6.0)
    assert need >= 7391 * 16
    base = 1 << 24
    x, work, out = (ctypes.c_void_p(base + k * (1 << 20)) for k in range(3))   # T = 8, C = 2: x 128 bytes, out 3 200, work ~118 KB

    def call(x=x, T=8, C=2, freqs=freqs, F=None, fps=100.0, omega0=5.0, radius=6.0, work=work, work_len=need, out=out, f32=0):
        F = (25 if freqs is None else len(freqs)) if F is None else F
        return lib.df3d_spectrogram(x, T, C, None if freqs is None else ptr(freqs), F, fps, omega0, radius, work, work_len, out, f32, None)

    def bank(freqs=freqs, F=None, fps=100.0, omega0=5.0, radius=6.0, work=work, work_len=need):
        F = len(freqs) if F is None else F
        return lib.df3d_spectrogram_bank(None if freqs is None else ptr(freqs), F, fps, omega0, radius, work, work_len, None)

    # no samples: nothing to do, whatever the pointers, and no device is needed
    assert lib.df3d_spectrogram(None, 0, 48, ptr(freqs), 25, 100.0, 5.0, 6.0, None, 0, None, 0, None) == 0
    assert call(T=-1) == -1 and b"T must be >= 0" in err()
    assert call(C=0) == -1 and b"C must be >= 1" in err()
    assert call(T=0, C=0) == -1 and b"C must be" in err()
    for F in (0, 65, -3):
        assert call(F=F) == -1 and b"F must be in [1, 64]" in err()
        assert bank(F=F) == -1 and b"F must be in [1, 64]" in err()
        assert lib.df3d_spectrogram_work_bytes(ptr(freqs), F, 100.0, 5.0, 6.0) == 0
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert call(fps=bad) == -1 and b"fps must be finite and > 0" in err(), bad
        assert call(omega0=bad) == -1 and b"omega0 must be finite and > 0" in err(), bad
        assert call(radius=bad) == -1 and b"radius must be finite and > 0" in err(), bad
        assert bank(fps=bad) == -1 and b"fps" in err()
        g = freqs.copy()
        g[0] = bad
        assert call(freqs=g) == -1 and b"f_min" in err(), bad
    assert call(freqs=freqs[::-1].copy()) == -1 and b"f_max < f_min" in err()
    g = freqs.copy()
    g[7] = np.nan
    assert call(freqs=g) == -1 and b"freqs[7]" in err()
    assert call(freqs=np.array([1.0, 50.5])) == -1 and b"f_max" in err() and b"fps/2" in err()
    assert lib.df3d_spectrogram_work_bytes(ptr(np.array([1.0, 50.0])), 2, 100.0, 5.0, 6.0) > 0   # fps / 2 itself is allowed
    assert call(freqs=None) == -1 and b"null pointer" in err()
    # K_0 = ceil(6 * 5 * 100 / (2 pi f)): 2048 fits, 2049 does not, and the message gives the frequency that does
    limit = 6.0 * 5.0 * 100.0 / (2.0 * np.pi * cfg.SPECTROGRAM_MAX_SUPPORT)
    assert lib.df3d_spectrogram_work_bytes(ptr(np.array([limit * (1 + 1e-12)])), 1, 100.0, 5.0, 6.0) >= 4097 * 16
    assert call(freqs=np.array([limit * 0.999, 2.0])) == -1 and b"cap of 2048" in err() and b"smallest f_min that fits is 0.2331" in err()
    assert call(freqs=np.array([1e-300])) == -1 and b"cap" in err()
    assert call(f32=2) == -1 and b"out_f32" in err()
    for name in ("x", "work", "out"):
        assert call(**{name: None}) == -1 and b"null pointer" in err(), name
    assert bank(work=None) == -1 and b"null pointer" in err()
    assert call(x=ctypes.c_void_p(base + 4)) == -1 and b"aligned" in err()
    assert call(out=ctypes.c_void_p(out.value + 4)) == -1 and b"aligned" in err()
    assert call(work=ctypes.c_void_p(work.value + 8)) == -1 and b"16-byte aligned" in err()
    assert bank(work=ctypes.c_void_p(work.value + 8)) == -1 and b"16-byte aligned" in err()
    assert call(work_len=need - 1) == -1 and b"work buffer too small" in err()
    assert bank(work_len=need - 1) == -1 and b"work buffer too small" in err()
    nx, no = 8 * 2 * 8, 8 * 2 * 25 * 8
    for o in (base, base + nx - 8, base - no + 8):
        assert call(out=ctypes.c_void_p(o)) == -1 and b"out must not overlap x" in err(), o
    for o in (base, base + nx - 16, base - need + 16, out.value, out.value + no - 16, out.value - need + 16):
        assert call(work=ctypes.c_void_p(o)) == -1 and b"work must not overlap" in err(), o
    assert call(T=1 << 40, C=1 << 20) == -1 and b"too large" in err()


# ------------------------------------------------------------------------------------------------------------------ ops
def test_ops_frequencies_and_support_match_the_oracle(native_lib):
    from deepfly3d_amd import ops

    for fps, kw in ((100.0, {}), (30.0, dict(f_min=1.0, f_max=7.5, num=8)), (250.0, dict(f_min=0.75, f_max=125.0, num=64)), (100.0, dict(num=1))):
        f = ops.wavelet_frequencies(fps, **kw)
        assert isinstance(f, np.ndarray) and f.dtype == np.float64
        assert np.array_equal(f, so.frequencies(fps, kw.get("f_min", 1.0), kw.get("f_max"), kw.get("num", 25)))
        K = ops.wavelet_support(fps, f)
        assert K.dtype == np.int64 and np.array_equal(K, so.support(fps, f))
    assert np.array_equal(ops.wavelet_support(100.0), so.support(100.0, so.frequencies(100.0)))
    assert np.array_equal(ops.wavelet_support(100.0, [2.0], omega0=6.0, radius=4.0), so.support(100.0, [2.0], 6.0, 4.0))


def test_ops_argument_errors(native_lib):
    import torch

    from deepfly3d_amd import ops

    for kw, what in ((dict(fps=0.0), "fps"), (dict(fps=np.nan), "fps"), (dict(f_min=0.0), "f_min"), (dict(f_min=np.inf), "f_min"), (dict(num=0), "num"),
                     (dict(num=65), "num"), (dict(f_min=5.0, f_max=4.0), "f_max"), (dict(f_max=50.5), "f_max"), (dict(f_max=np.nan), "f_max")):
        with pytest.raises(ValueError, match=what):
            ops.wavelet_frequencies(**{"fps": 100.0, **kw})
    x = torch.zeros((10, 2), dtype=torch.float64)   # on the host: refused, but only after the bank has been checked
    for kw, what in ((dict(freqs=[[1.0]]), "freqs"), (dict(freqs=["a"]), "freqs"), (dict(freqs=[2.0, 1.0]), "f_max < f_min"), (dict(freqs=[60.0]), "fps/2"),
                     (dict(freqs=[0.1]), "smallest f_min that fits"), (dict(omega0=0.0), "omega0"), (dict(radius=-1.0), "radius"),
                     (dict(freqs=np.ones(65)), "F must be"), (dict(freqs=[]), "F must be"), (dict(dtype=torch.float16), "dtype")):
        with pytest.raises(ValueError, match=what):
            ops.wavelet_spectrogram(x, 100.0, **kw)
    with pytest.raises(ValueError, match="fps"):
        ops.wavelet_spectrogram(x, -5.0)
    with pytest.raises(ValueError, match="series"):
        ops.wavelet_spectrogram(x, 100.0)
    with pytest.raises(ValueError, match="smallest f_min"):
        ops.wavelet_support(100.0, [0.1])


def test_unwrap_rule_matches_numpy(native_lib):
    import torch

    from deepfly3d_amd import ops

    rng = np.random.default_rng(5)
    T = 400
    walk = np.cumsum(rng.uniform(-2.0, 2.0, size=(T, 6)), axis=0)            # wanders over many turns
    wrapped = np.angle(np.exp(1j * walk))
    wrapped[:, 5] = np.linspace(0, 40, T) % (2 * np.pi) - np.pi               # a saw-tooth
    wrapped[10, 4], wrapped[11, 4] = -np.pi / 2, np.pi / 2                    # a step of exactly pi
    out, left = ops.unwrap_phase(torch.from_numpy(wrapped))
    assert left == [] and np.abs(out.numpy() - np.unwrap(wrapped, axis=0)).max() <= 1e-12
    # only the requested columns move; a column with a non-finite sample is left as it is and reported
    bad = wrapped.copy()
    bad[77, 2], bad[5, 3] = np.nan, np.inf
    out, left = ops.unwrap_phase(torch.from_numpy(bad), [0, 2, 3, 5])
    assert left == [2, 3]
    got = out.numpy()
    assert np.array_equal(got[:, [1, 4]], bad[:, [1, 4]]) and got[:, [2, 3]].tobytes() == bad[:, [2, 3]].tobytes()
    assert np.abs(got[:, [0, 5]] - np.unwrap(wrapped[:, [0, 5]], axis=0)).max() <= 1e-12
    one = torch.from_numpy(wrapped[:1])
    assert np.array_equal(ops.unwrap_phase(one)[0].numpy(), wrapped[:1]) and ops.unwrap_phase(torch.zeros((0, 3), dtype=torch.float64))[0].shape == (0, 3)
    with pytest.raises(ValueError, match="series"):
        ops.unwrap_phase(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="channels"):
        ops.unwrap_phase(torch.from_numpy(wrapped), [6])


# ------------------------------------------------------------------------------------------------------------------ config, CLI, Core
def test_config_defaults():
    from deepfly3d_amd import config as cfg

    assert (cfg.SPECTROGRAM_F_MIN, cfg.SPECTROGRAM_F_MAX_OVER_FPS, cfg.SPECTROGRAM_NUM_FREQS) == (so.F_MIN, so.F_MAX_OVER_FPS, so.NUM_FREQS) == (1.0, 0.25, 25)
    assert (cfg.SPECTROGRAM_OMEGA0, cfg.SPECTROGRAM_RADIUS, cfg.SPECTROGRAM_FPS) == (so.OMEGA0, so.RADIUS, 100.0) == (5.0, 6.0, 100.0)
    assert cfg.SPECTROGRAM_MAX_SUPPORT >= 2048
    assert cfg.SPECTROGRAM_UNWRAPPED_ANGLES == ("thc_pitch", "thc_roll", "ctr_roll", "fti_roll")
    assert all(a in cfg.LEG_ANGLE_NAMES for a in cfg.SPECTROGRAM_UNWRAPPED_ANGLES)


def test_cli_flag_parses_and_counts_as_something_to_do(tmp_path, monkeypatch):
    from deepfly3d_amd import cli

    assert cli.parse_cli_args(["/tmp/x", "--angle-spectrogram"]).angle_spectrogram is True
    assert cli.parse_cli_args(["/tmp/x"]).angle_spectrogram is False
    args = cli.parse_cli_args(["/tmp/x", "--angle-spectrogram", "--rigid-legs", "--skip-pose-estimation"])
    assert args.angle_spectrogram and args.rigid_legs and not args.joint_angles and args.skip_estimation

    class Reached(Exception):
        pass

    def core(*a, **kw):
        raise Reached()

    monkeypatch.setattr(cli, "Core", core)
    assert cli.run(cli.parse_cli_args([str(tmp_path), "--skip-pose-estimation"])) == 0
    with pytest.raises(Reached):
        cli.run(cli.parse_cli_args([str(tmp_path), "--skip-pose-estimation", "--angle-spectrogram"]))


def test_cli_flag_without_a_result_to_reopen_is_refused(tmp_path, golden_dir):
    from deepfly3d_amd import cli
    from deepfly3d_amd.config import config

    folder = tmp_path / "images"   # one frame per camera and no earlier result: nothing to calibrate or triangulate
    folder.mkdir()
    for c in range(7):
        os.symlink(os.path.join(golden_dir, "images", f"camera_{c}_img_0.jpg"), folder / f"camera_{c}_img_0.jpg")
    config.pop("image_shape", None)
    args = cli.parse_cli_args([str(folder), "--angle-spectrogram", "--skip-pose-estimation"])
    with pytest.raises(RuntimeError, match="--angle-spectrogram needs calibrated cameras"):
        cli.run(args)
    config.pop("image_shape", None)
    assert not [f for f in os.listdir(str(folder) + "_df3d") if f.startswith("df3d_result")]


class _Net:
    def __init__(self, calibrated):
        self.calibrated, self.points3d = calibrated, None

    def has_calibration(self):
        return self.calibrated


def _bare_core(tmp_path=None):
    from deepfly3d_amd.core import Core

    core = Core.__new__(Core)
    core.camNet, core.device, core.is_primary = _Net(False), "cpu", True
    core.get_fps = lambda: None
    return core


def test_core_angle_spectrogram_refusals(monkeypatch):
    from deepfly3d_amd import distributed as dd

    core = _bare_core()
    for net in (_Net(False), None):
        core.camNet = net
        with pytest.raises(RuntimeError, match=r"angle_spectrogram needs calibrated cameras: run calibrate_calc\(\)"):
            core.angle_spectrogram()
        with pytest.raises(RuntimeError, match=r"calibrate_calc\(\)"):
            core.angle_spectrogram(rigid=True)
    core.camNet = _Net(True)
    with pytest.raises(TypeError, match="window"):
        core.angle_spectrogram(window=3)
    with pytest.raises(TypeError, match="either freqs or"):
        core.angle_spectrogram(freqs=[1.0], num=3)
    with pytest.raises(ValueError, match="f_max"):
        core.angle_spectrogram(fps=20.0, f_max=11.0)
    monkeypatch.setattr(dd, "current", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="angle_spectrogram is a rank-0"):
        core.angle_spectrogram()


def test_result_written_without_the_flag_is_unchanged(tmp_path):
    """The bytes of a result pickle do not depend on the new argument as long as it is off; with it on and no cameras the save is refused
    before anything is written."""
    core = _bare_core()
    core.camNet = None
    core.points2d = np.arange(7 * 3 * 19 * 2, dtype=np.float64).reshape(7, 3, 19, 2)
    core.points2d_argmax, core.camera_ordering, core.conf = None, np.arange(7), np.ones((7, 3, 19))
    (tmp_path / "in").mkdir()
    core.output_folder, core.input_folder = str(tmp_path), str(tmp_path / "in")
    core._write_result()
    with open(core.save_path, "rb") as f:
        plain = f.read()
    assert list(pickle.loads(plain).keys()) == ["points2d", "camera_ordering", "heatmap_confidence"]
    core._write_result(None, False, False, False)
    with open(core.save_path, "rb") as f:
        assert f.read() == plain
    os.remove(core.save_path)
    with pytest.raises(RuntimeError, match="angle_spectrogram needs calibrated cameras"):
        core._write_result(angle_spectrogram=True)
    assert not os.path.exists(core.save_path)
