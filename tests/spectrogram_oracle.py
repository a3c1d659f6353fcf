"""The Morlet wavelet spectrogram of DESIGN.md section 16 in numpy float64: the definition the HIP kernel (csrc/spectrogram.hip) is
tested against, written as the plain sum over the taps, plus an independent witness that convolves the edge-extended series with
scipy.signal.fftconvolve.  Not a port of anything: the model is this project's own specification.

    x [T, C] float64, fps > 0, frequencies f_i (Hz), omega0, radius
    sigma_i = omega0 fps / (2 pi f_i),  K_i = ceil(radius sigma_i)
    k = -K_i..K_i:  g = exp(-k^2 / (2 sigma_i^2)),  phi = 2 pi f_i k / fps
    kappa_i = sum g cos phi / sum g,  n_i = 2 / sum g
    a_i[k] = n_i g (cos phi - kappa_i),  b_i[k] = -n_i g sin phi
    A = sum_k a_i[k] x[clamp(t + k, 0, T - 1), c],  B likewise with b_i
    S[t, c, i] = sqrt(A^2 + B^2), NaN where A or B is not finite
"""
import numpy as np

F_MIN, F_MAX_OVER_FPS, NUM_FREQS, OMEGA0, RADIUS = 1.0, 0.25, 25, 5.0, 6.0


def frequencies(fps, f_min=F_MIN, f_max=None, num=NUM_FREQS):
    f_max = fps * F_MAX_OVER_FPS if f_max is None else f_max
    if num == 1:
        return np.array([f_min], dtype=np.float64)
    f = f_min * (f_max / f_min) ** (np.arange(num, dtype=np.float64) / (num - 1))
    f[-1] = f_max
    return f


def support(fps, freqs, omega0=OMEGA0, radius=RADIUS):
    sigma = omega0 * fps / (2.0 * np.pi * np.asarray(freqs, dtype=np.float64))
    return np.ceil(radius * sigma).astype(np.int64)


def taps(fps, f, omega0=OMEGA0, radius=RADIUS, admissible=True):
    """(K, a [2K + 1], b [2K + 1]) of one row.  `admissible=False` leaves kappa out (what a constant offset then leaks is a test)."""
    sigma = omega0 * fps / (2.0 * np.pi * f)
    K = int(np.ceil(radius * sigma))
    k = np.arange(-K, K + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    phi = 2.0 * np.pi * f * k / fps
    kappa = np.sum(g * np.cos(phi)) / np.sum(g) if admissible else 0.0
    n = 2.0 / np.sum(g)
    return K, n * g * (np.cos(phi) - kappa), -n * g * np.sin(phi)


def _finish(A, B):
    with np.errstate(all="ignore"):
        S = np.sqrt(A * A + B * B)
    S[~(np.isfinite(A) & np.isfinite(B))] = np.nan
    return S


def spectrogram(x, fps, freqs=None, omega0=OMEGA0, radius=RADIUS, admissible=True):
    """S [T, C, F] float64 of x [T, C] (or [T]): the definition, one tap after the other from k = -K_i to K_i."""
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(x.shape[0], int(np.prod(x.shape[1:])))
    T, C = flat.shape
    freqs = frequencies(fps) if freqs is None else np.asarray(freqs, dtype=np.float64)
    S = np.empty((T, C, len(freqs)), dtype=np.float64)
    t = np.arange(T)
    with np.errstate(all="ignore"):
        for i, f in enumerate(freqs):
            K, a, b = taps(fps, f, omega0, radius, admissible)
            A, B = np.zeros((T, C)), np.zeros((T, C))
            for k in range(-K, K + 1):
                xs = flat[np.clip(t + k, 0, T - 1)] if T else flat
                A += a[k + K] * xs
                B += b[k + K] * xs
            S[:, :, i] = _finish(A, B)
    return S.reshape(*x.shape, len(freqs))


def witness(x, fps, freqs=None, omega0=OMEGA0, radius=RADIUS):
    """The same amplitudes by another route: the series extended by K_i edge samples on either side and convolved with the
    reversed taps by scipy.signal.fftconvolve.  Finite series only (an FFT spreads a NaN everywhere)."""
    from scipy.signal import fftconvolve

    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(x.shape[0], int(np.prod(x.shape[1:])))
    T, C = flat.shape
    freqs = frequencies(fps) if freqs is None else np.asarray(freqs, dtype=np.float64)
    S = np.empty((T, C, len(freqs)), dtype=np.float64)
    for i, f in enumerate(freqs):
        K, a, b = taps(fps, f, omega0, radius)
        ext = np.concatenate([np.repeat(flat[:1], K, axis=0), flat, np.repeat(flat[-1:], K, axis=0)], axis=0)
        A = fftconvolve(ext, a[::-1, None], mode="valid", axes=0)
        B = fftconvolve(ext, b[::-1, None], mode="valid", axes=0)
        S[:, :, i] = np.sqrt(A * A + B * B)
    return S.reshape(*x.shape, len(freqs))


def tolerance(x, fps, freqs, omega0=OMEGA0, radius=RADIUS):
    """[C, F]: the bound on |device - oracle| per element, 16 (2 K_i + 64) 2^-53 max_t |x[:, c]| (section 16 derives it: the
    worst-case rounding of the two sums, (2 K_i + 1) eps 2 max|x|, plus the taps' own error of about 35 eps each, times four)."""
    flat = np.asarray(x, dtype=np.float64).reshape(x.shape[0], int(np.prod(x.shape[1:])))
    with np.errstate(all="ignore"):
        peak = np.max(np.where(np.isfinite(flat), np.abs(flat), 0.0), axis=0) if flat.shape[0] else np.zeros(flat.shape[1])
    K = support(fps, freqs, omega0, radius)
    return 16.0 * (2.0 * K[None, :] + 64.0) * 2.0 ** -53 * peak[:, None]
