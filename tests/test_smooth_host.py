"""CPU tests of the temporal smoothing of 2-D detections: the float64 oracle tests/smooth_oracle.py against
outputs of the reference's own `smooth_pose2d` (tests/golden/smooth_golden.npz), the coefficient builder, the argument validation
of df3d_smooth_pose2d (no device is touched), and the CLI flag."""
import ctypes

import numpy as np
import pytest

import smooth_oracle as so

# the collapsed form against scipy's own summation order: 57 folded taps on values <= 1 000 px in float64, 57 * 2^-53 * 1000 = 6e-12
ORACLE_ATOL = 1e-11


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(f"{golden_dir}/smooth_golden.npz")


def test_oracle_reproduces_the_reference(golden):
    assert sorted(int(t) for t in golden["lengths"]) == [1, 2, 9, 21, 400]
    for T in golden["lengths"]:
        inp, out, std = golden[f"inp_{T}"], golden[f"out_{T}"], golden[f"std_{T}"]
        assert inp.shape == (T, 38, 2)
        got = so.smooth_pose2d(inp)
        print(T, "max |oracle - reference|", np.abs(got - out).max(), "min |std - 5|", np.abs(std - 5.0).min())
        assert np.abs(got - out).max() <= ORACLE_ATOL
        assert np.abs(so.window_std(inp.reshape(T, 76)).reshape(T, 38, 2) - std).max() <= 1e-11
        assert np.abs(std - 5.0).min() > 1e-9   # the fixtures hold no threshold cell: the reference's branch is unambiguous


def test_fixture_exercises_both_branches_and_unseen_joints(golden):
    inp, out, std = golden["inp_400"], golden["out_400"], golden["std_400"]
    lively = std >= 5.0
    assert 0.05 < lively.mean() < 0.5 and lively[100:160].mean() > 0.9
    assert np.array_equal(out[lively], inp[lively])                  # sigma 0.1: the sample itself
    seen = np.ones(38, dtype=bool)
    seen[5] = False
    assert (out[:, seen][~lively[:, seen]] != inp[:, seen][~lively[:, seen]]).mean() > 0.9   # sigma 7: an average
    assert not inp[:, 5].any() and not out[:, 5].any()               # an unseen joint stays at zero
    assert not inp[200:260, 23].any() and not out[210:250, 23].any() and out[199, 23].all()


def test_coefficient_builder():
    from deepfly3d_amd import ops

    for w in (2, 20, 64):
        taps = ops.gaussian_window_taps(w, 7.0)
        assert taps.shape == (w,) and abs(taps.sum() - 1.0) <= 1e-15 and (taps[max(0, w // 2 - 28):w // 2 + 29] > 0).all()
        assert np.abs(taps - so.window_taps(w, 7.0)).max() <= 1e-16
        keep = ops.gaussian_window_taps(w, 0.1)
        assert np.array_equal(keep, np.eye(w)[w // 2])               # sigma 0.1: radius 0, the identity
    taps = ops.gaussian_window_taps(20, 7.0)
    # interior taps are the Gaussian's own, symmetric about the centre (index 10); the two end samples collect the folded tails,
    # the last one more of them: it lies 9 samples from the centre, the first one 10
    assert np.array_equal(taps[10 + np.arange(1, 9)], taps[10 - np.arange(1, 9)]) and taps[9] == taps[11] < taps[10]
    assert taps[19] > taps[0] and np.all(np.diff(taps[1:11]) > 0) and taps[0] > taps[1] and taps[19] > taps[18]
    # a window wider than the filter folds nothing: 57 taps inside 128 samples
    wide = ops.gaussian_window_taps(128, 7.0)
    assert np.count_nonzero(wide) == 57 and np.array_equal(wide[64 - 28:64 + 29], wide[64 - 28:64 + 29][::-1])
    with pytest.raises(ValueError):
        ops.gaussian_window_taps(20, 0.0)


def test_oracle_rules():
    rng = np.random.default_rng(5)
    x = 300.0 + np.cumsum(rng.normal(0, 1.0, size=(60, 4)), axis=0)
    out, std = so.smooth(x, 20, 5.0)
    assert (std < 5.0).all() and np.abs(out - x).max() > 0.1
    # the threshold is strict: std == thr keeps
    flat = np.tile(np.array([0.0, 10.0] * 30)[:, None], (1, 2))     # every window: ten 0s and ten 10s, std exactly 5
    kept, std = so.smooth(flat, 20, 5.0)
    assert np.array_equal(std[10:50], np.full((40, 2), 5.0)) and np.array_equal(kept[10:50], flat[10:50])
    assert not np.array_equal(so.smooth(flat, 20, np.nextafter(5.0, 6.0))[0][10:50], flat[10:50])
    # a NaN or an infinity: every window that holds it keeps its centre sample, the others are untouched by it
    y = x.copy()
    y[30, 1], y[40, 2] = np.nan, np.inf
    got, _ = so.smooth(y, 20, 5.0)
    for t, ch in ((30, 1), (40, 2)):
        held = np.arange(t - 9, t + 11)                              # windows t' - 10 .. t' + 9 that hold frame t
        assert np.array_equal(np.delete(got[held, ch], 9), np.delete(y[held, ch], 9))
        assert np.isnan(got[t, ch]) if np.isnan(y[t, ch]) else got[t, ch] == y[t, ch]
        rest = np.setdiff1d(np.arange(60), held)
        assert np.array_equal(got[rest, ch], out[rest, ch])
    # edge replication: a one-frame series is a constant window, its average the frame (the taps sum to 1 within an ulp); no frames, no output
    assert np.abs(so.smooth(x[:1], 20, 5.0)[0] - x[:1]).max() <= 1e-12
    assert so.smooth(np.zeros((0, 6)), 20, 5.0)[0].shape == (0, 6)


def test_smooth_entry_validates_arguments_without_gpu(native_lib):
    from deepfly3d_amd import _native

    ok = (ctypes.c_double * 64)(*([1.0 / 20] * 20))
    nan = (ctypes.c_double * 64)(*([float("nan")] * 64))
    inf = (ctypes.c_double * 64)(*([float("inf")] * 64))
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)

    def call(pts=p, C=7, T=100, nch=76, window=20, thr=5.0, ws=ok, wk=ok, out=q):
        return native_lib.df3d_smooth_pose2d(pts, C, T, nch, window, thr, ws, wk, out, None)

    for bad, word in ((dict(C=0), b"C must"), (dict(C=9), b"C must"), (dict(nch=0), b"nch"), (dict(nch=129), b"nch"), (dict(window=0), b"window"),
                      (dict(window=21), b"window"), (dict(window=66), b"window"), (dict(thr=-1.0), b"std_thr"), (dict(thr=float("nan")), b"std_thr"),
                      (dict(T=-1), b"T must"), (dict(ws=None), b"null"), (dict(wk=None), b"null"), (dict(ws=nan), b"finite"), (dict(wk=inf), b"finite"),
                      (dict(pts=None), b"null"), (dict(out=None), b"null"), (dict(out=p), b"alias"),
                      (dict(out=ctypes.c_void_p((1 << 20) + 8 * 7 * 100 * 76 - 8)), b"alias"), (dict(pts=ctypes.c_void_p((1 << 30) + 8)), b"alias")):
        assert call(**bad) == _native.DF3D_EINVAL, bad
        assert word in native_lib.df3d_last_error(), (bad, native_lib.df3d_last_error())
    assert call(T=0, pts=None, out=None) == 0            # an empty recording: nothing to do
    assert call(T=0, window=21) == _native.DF3D_EINVAL   # ... but still a checked call


def test_cli_smooth_2d_needs_video_2d(capsys):
    from deepfly3d_amd import cli

    with pytest.raises(SystemExit):
        cli.parse_cli_args(["/tmp/x", "--smooth-2d"])
    assert "--video-2d" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_cli_args(["/tmp/x", "--smooth-2d", "--video-3d"])
    args = cli.parse_cli_args(["/tmp/x", "--video-2d", "--smooth-2d"])
    assert args.smooth_2d and args.video_2d
    assert cli.parse_cli_args(["/tmp/x", "--video-2d"]).smooth_2d is False


def test_smooth_signatures():
    import inspect

    from deepfly3d_amd import ops, video
    from deepfly3d_amd.core import Core

    assert list(inspect.signature(ops.smooth_pose2d).parameters) == ["points2d", "window_size", "std_thr"]
    assert inspect.signature(ops.smooth_pose2d).parameters["window_size"].default == 20
    assert inspect.signature(ops.smooth_pose2d).parameters["std_thr"].default == 5.0
    assert list(inspect.signature(Core.smooth_points2d).parameters) == ["self", "cam_id", "refresh"]   # no shared private_cache
    assert inspect.signature(video.make_pose2d_video).parameters["smooth"].default is False
