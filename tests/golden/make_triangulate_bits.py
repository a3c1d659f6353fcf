"""Writes tests/golden/triangulate_bits.npz: inputs and outputs of df3d_triangulate from the library as it was BEFORE the DLT
code moved into csrc/geometry_dev.h (shared with the pictorial-structures proposals), so that the move is checked bit for bit.
Run once on the GPU with that earlier build:  DF3D_LIB=<earlier libdf3d_hip.so> python tests/golden/make_triangulate_bits.py OUT

Cases: the golden 2-D detections through the golden cameras, and 32 frames of random pixels (some views zeroed = unseen)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import geometry as og  # noqa: E402


def cases():
    g2, g3 = np.load(os.path.join(HERE, "golden_2d.npz")), np.load(os.path.join(HERE, "golden_3d.npz"))
    P = og.projection_matrices(g3["R"], g3["tvec"], g3["intr"])
    golden = og.pixels_from_normalised(g2["points2d"], [960, 480])
    rng = np.random.default_rng(20261015)
    rand = rng.uniform(1.0, 900.0, size=(7, 32, 38, 2))
    rand[rng.random((7, 32, 38)) < 0.3] = 0.0
    return P, golden, rand


def _triangulate(lib, P, px, dev):
    """df3d_triangulate through ctypes alone: an earlier build lacks entries the current bindings (_native.PROTOTYPES) declare."""
    import ctypes

    pts = torch.from_numpy(np.ascontiguousarray(px)).to(dev)
    ncam, T, J, _ = pts.shape
    X = torch.empty((T, J, 3), dtype=torch.float64, device=dev)
    Ph = np.ascontiguousarray(P, dtype=np.float64)
    fn = lib.df3d_triangulate
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(Ph.ctypes.data_as(ctypes.c_void_p), pts.data_ptr(), ncam, T, J, X.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
    return X.cpu().numpy()


def main(out):
    import ctypes

    from deepfly3d_amd import _native

    P, golden, rand = cases()
    dev = torch.device("cuda:0")
    lib = ctypes.CDLL(_native.library_path())
    X = [_triangulate(lib, P, p, dev) for p in (golden, rand)]
    np.savez_compressed(out, P=P, golden_px=golden, random_px=rand, golden_X=X[0], random_X=X[1])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "triangulate_bits.npz"))
