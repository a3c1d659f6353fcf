"""Device time of the wavelet spectrogram: df3d_spectrogram on --frames samples of 48 channels with the default
bank at 100 fps (25 rows, K = 478..20, 7 391 taps), float64 and float32 output, timed with device events (20 launches after 3
warm-ups), beside the bank kernel's own time, the flop model (2 T C sum(2 K_i + 1) multiply-adds at the 78.6 Tflop/s float64 vector
peak) and the byte model (every tile's samples with their halo read once, the output written once, at 8 TB/s).  --witness also
times the FFT witness of tests/spectrogram_oracle.py on the host for the same problem, for scale.

    python tests/perf/bench_spectrogram.py [--frames 1000 100000] [--witness] [--out result.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from deepfly3d_amd import _native, config, ops  # noqa: E402

HBM = 8e12                 # bytes per second
FP64_VECTOR = 78.6e12      # flop per second, vector float64 with every operation a multiply-add
C = 48
FPS = 100.0


def series(T):
    rng = np.random.default_rng(16)
    t = np.arange(T)[:, None]
    return rng.standard_normal((T, C)) + np.sin(2 * np.pi * (1.0 + np.arange(C)[None, :] % 12) * t / FPS)


def timed(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps   # us per launch


def kernels(T, dev):
    lib = _native.load()
    freqs = ops.wavelet_frequencies(FPS)
    K = ops.wavelet_support(FPS, freqs)
    taps = int(np.sum(2 * K + 1))
    tile = config.SPECTROGRAM_TILE
    x = torch.from_numpy(series(T)).to(dev).t().contiguous()
    fp = freqs.ctypes.data_as(ctypes.c_void_p)
    need = lib.df3d_spectrogram_work_bytes(fp, len(freqs), FPS, config.SPECTROGRAM_OMEGA0, config.SPECTROGRAM_RADIUS)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    bank_args = (fp, len(freqs), FPS, config.SPECTROGRAM_OMEGA0, config.SPECTROGRAM_RADIUS)

    def bank():
        _native.check(lib.df3d_spectrogram_bank(*bank_args, work.data_ptr(), need, stream), "df3d_spectrogram_bank")

    tiles = (T + tile - 1) // tile
    flop = 2.0 * 2.0 * T * C * taps
    res = {"frames": T, "channels": C, "rows": len(freqs), "taps": taps, "grid": [tiles * C, 256], "flop": flop,
           "flop_model_us": flop / FP64_VECTOR * 1e6, "bank_us": timed(bank), "output": {}}
    for name, dtype in (("float64", torch.float64), ("float32", torch.float32)):
        out = torch.empty((T, C, len(freqs)), dtype=dtype, device=dev)

        def run():
            _native.check(lib.df3d_spectrogram(x.data_ptr(), T, C, *bank_args, work.data_ptr(), need, out.data_ptr(), int(dtype == torch.float32),
                                               stream), "df3d_spectrogram")

        us = timed(run)
        nbytes = tiles * C * (tile + 2 * int(K.max())) * 8 + out.numel() * out.element_size()
        res["output"][name] = {"us": us, "us_per_1000_frames": us * 1000.0 / T, "fraction_of_fp64_vector_peak": flop / (us * 1e-6) / FP64_VECTOR,
                               "bytes": nbytes, "byte_model_us": nbytes / HBM * 1e6, "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM}
    return res


def witness_seconds(T):
    import spectrogram_oracle as so

    x = series(T)
    t0 = time.perf_counter()
    so.witness(x, FPS)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--witness", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "kernels": [kernels(T, dev) for T in a.frames]}
    if a.witness:
        res["host_fft_witness_seconds"] = {str(T): witness_seconds(T) for T in a.frames}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
