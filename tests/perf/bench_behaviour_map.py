"""Device time of every stage of the behaviour map at N = 2 048 and 8 192 training frames of D = 1 200 channels,
and of the placement of --frames (100 000) further frames against the larger set, timed with device events (several launches after
warm-ups), each beside a flop model (at the 78.6 Tflop/s float64 vector peak, every operation counted as half a multiply-add) and a
byte model (every operand read once, every result written once, at 8 TB/s).  The calibration's flop model ASSUMES 12 root steps of
30 flop per entry (an exponential and three multiply-adds); the kernel does not report its count.  --witness times scikit-learn's
exact t-SNE on the host at N = 2 048 for scale, where it is installed; --witness-only needs no device.

    python tests/perf/bench_behaviour_map.py [--points 2048 8192] [--frames 100000] [--witness] [--out result.json]
"""
import argparse
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
D = 1200
PAIR_FLOP = 22             # per pair of the gradient: two differences, 1 + |d|^2, the reciprocal (about ten), two products, five sums
ROOT_STEPS, ENTRY_FLOP = 12, 30


def spectra(T, seed=17):
    """[T, D] spectra round eight centres (a silent tenth of the channels)."""
    rng = np.random.default_rng(seed)
    base = rng.gamma(2.0, 1.0, size=(8, D)) * (rng.random((8, D)) > 0.1)
    return base[rng.integers(0, 8, size=T)] * np.exp(0.3 * rng.standard_normal((T, D)))


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps   # us per call


def entry(us, flop, nbytes):
    return {"us": us, "flop": flop, "flop_model_us": flop / FP64_VECTOR * 1e6, "fraction_of_fp64_vector_peak": flop / (us * 1e-6) / FP64_VECTOR,
            "bytes": nbytes, "byte_model_us": nbytes / HBM * 1e6, "fraction_of_8TBps": nbytes / (us * 1e-6) / HBM}


def stages(N, dev):
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    u, tol, bmax = config.BEHAVIOUR_PERPLEXITY, config.BEHAVIOUR_ENTROPY_TOL, config.BEHAVIOUR_BETA_MAX
    S = torch.from_numpy(spectra(N)).to(dev)
    p, logp = torch.empty_like(S), torch.empty_like(S)
    e = torch.empty((N,), dtype=torch.float64, device=dev)
    valid = torch.empty((N,), dtype=torch.int32, device=dev)
    K, cond, P = (torch.empty((N, N), dtype=torch.float64, device=dev) for _ in range(3))
    beta = torch.empty((N,), dtype=torch.float64, device=dev)
    info = torch.empty((N,), dtype=torch.int32, device=dev)
    me = torch.arange(N, dtype=torch.int32, device=dev)
    need = lib.df3d_bmap_work_bytes(N)
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    cost = torch.empty((1,), dtype=torch.float64, device=dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    Y = (1e-4 * torch.randn((N, 2), generator=gen, dtype=torch.float64)).to(dev)
    V, G = torch.zeros_like(Y), torch.ones_like(Y)
    check = _native.check
    res = {"points": N, "channels": D}
    res["prepare"] = entry(timed(lambda: check(lib.df3d_bmap_prepare(S.data_ptr(), N, D, config.BEHAVIOUR_FLOOR, p.data_ptr(), logp.data_ptr(),
                                                                       e.data_ptr(), valid.data_ptr(), stream))), 30.0 * N * D, 3 * N * D * 8)
    res["divergence"] = entry(timed(lambda: check(lib.df3d_bmap_divergence(p.data_ptr(), e.data_ptr(), N, logp.data_ptr(), N, D, K.data_ptr(), stream))),
                              2.0 * N * N * D, (2 * N * D + N * N) * 8)
    res["calibrate"] = entry(timed(lambda: check(lib.df3d_bmap_calibrate(K.data_ptr(), N, N, u, tol, bmax, me.data_ptr(), cond.data_ptr(), beta.data_ptr(),
                                                                         info.data_ptr(), stream))), float(ROOT_STEPS * ENTRY_FLOP) * N * N, 2 * N * N * 8)
    res["calibrate"]["rows_that_tie"] = int((info & 1).sum())
    res["joint"] = entry(timed(lambda: check(lib.df3d_bmap_joint(cond.data_ptr(), N, P.data_ptr(), stream))), 2.0 * N * N, 3 * N * N * 8)
    iters = 20
    lr = max(N / 48.0, 50.0)
    for name, first in (("iteration_exaggerated", 0), ("iteration_late", 400)):
        us = timed(lambda: check(lib.df3d_tsne_run(P.data_ptr(), N, Y.data_ptr(), V.data_ptr(), G.data_ptr(), first, iters, lr, work.data_ptr(), need,
                                                   stream))) / iters
        res[name] = entry(us, float(PAIR_FLOP) * N * N, N * N * 8 + N * 16 * (N // 1024 + 1))
    res["cost"] = entry(timed(lambda: check(lib.df3d_bmap_cost(P.data_ptr(), N, Y.data_ptr(), cost.data_ptr(), work.data_ptr(), need, stream))),
                        60.0 * N * N, N * N * 8)
    res["descent_of_1000_iterations_ms"] = (config.BEHAVIOUR_EXAGGERATION_ITERATIONS * res["iteration_exaggerated"]["us"]
                                            + (1000 - config.BEHAVIOUR_EXAGGERATION_ITERATIONS) * res["iteration_late"]["us"]) * 1e-3
    return res, (p, logp, e, Y)


def placement(T, train, dev):
    """T frames placed against the training set `train` = (p, logp, e, Y): the row chunks ops.behaviour_map walks."""
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    _, lt, _, Y = train
    N = lt.shape[0]
    chunk = max(1, ops._PLACE_CHUNK_BYTES // (8 * N))
    S = torch.from_numpy(spectra(min(T, chunk), seed=18)).to(dev)
    p, logp, e, valid = ops._distributions(S)
    rows = p.shape[0]
    K, cond = (torch.empty((rows, N), dtype=torch.float64, device=dev) for _ in range(2))
    beta = torch.empty((rows,), dtype=torch.float64, device=dev)
    info = torch.empty((rows,), dtype=torch.int32, device=dev)
    out = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    check = _native.check
    u, tol, bmax = config.BEHAVIOUR_PERPLEXITY, config.BEHAVIOUR_ENTROPY_TOL, config.BEHAVIOUR_BETA_MAX
    chunks = (T + rows - 1) // rows   # the same chunk timed again: the data differ, the work does not
    parts = {
        "divergence": (lambda: check(lib.df3d_bmap_divergence(p.data_ptr(), e.data_ptr(), rows, lt.data_ptr(), N, D, K.data_ptr(), stream)),
                       2.0 * rows * N * D, (rows * D + N * D + rows * N) * 8),
        "calibrate": (lambda: check(lib.df3d_bmap_calibrate(K.data_ptr(), rows, N, u, tol, bmax, None, cond.data_ptr(), beta.data_ptr(), info.data_ptr(),
                                                            stream)), float(ROOT_STEPS * ENTRY_FLOP) * rows * N, 2 * rows * N * 8),
        "place": (lambda: check(lib.df3d_bmap_place(cond.data_ptr(), rows, N, Y.data_ptr(), out.data_ptr(), stream)), 4.0 * rows * N, rows * N * 8),
    }
    res = {"frames": T, "points": N, "rows_per_chunk": rows, "chunks": chunks}
    total = 0.0
    for name, (fn, flop, nbytes) in parts.items():
        res[name] = entry(timed(fn, warmup=1, reps=3) * chunks, flop * chunks, nbytes * chunks)
        total += res[name]["us"]
    res["total_ms"] = total * 1e-3
    return res


def witness_seconds(N=2048):
    """scikit-learn's exact t-SNE (1 000 iterations, precomputed divergences made symmetric) on the host, for scale."""
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return None
    import behaviour_map_oracle as bo

    p = bo.distributions(spectra(N))[0]
    L = np.log(p)
    K = np.maximum((p * L).sum(axis=1)[:, None] - p @ L.T, 0.0)
    K = 0.5 * (K + K.T)
    np.fill_diagonal(K, 0.0)
    t0 = time.perf_counter()
    TSNE(method="exact", metric="precomputed", init="random", perplexity=config.BEHAVIOUR_PERPLEXITY, random_state=0).fit_transform(K)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--witness", action="store_true")
    ap.add_argument("--witness-only", dest="witness_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.witness_only:
        dev = torch.device("cuda:0")
        res["device"] = torch.cuda.get_device_name(0)
        res["stages"] = []
        train = None
        for N in a.points:
            r, train = stages(N, dev)
            res["stages"].append(r)
        if a.frames > 0:
            res["placement"] = placement(a.frames, train, dev)
    if a.witness or a.witness_only:
        res["host_sklearn_exact_tsne_seconds_at_2048"] = witness_seconds()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
