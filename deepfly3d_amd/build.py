"""Build libdf3d_hip.so for gfx950 in-tree with hipcc (cross-compiles without a GPU).

    python -m deepfly3d_amd.build [--force] [--verbose]

The shared library lands next to this file so it travels with the source snapshot to the GPU box.
"""
import argparse
import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ_DIR = os.path.join(HERE, "csrc", "_obj")
LIB_PATH = os.path.join(HERE, "libdf3d_hip.so")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function", "-ffp-contract=fast"]
# pose3d.hip and ba_lsmr.hip reproduce float64 scalar recurrences (One-Euro filter, LSMR rotations) exactly as the
# CPU reference arithmetic rounds them: no multiply-add fusion there
# render.hip (f4, the video frames): float64 pixel tests restated in numpy by oracle/render.py, compared bit for bit
#   (and the heat-map overlay of DESIGN.md section 13, restated in tests/heatmap_overlay_oracle.py)
# smooth.hip keeps the default -ffp-contract=fast on purpose: its test bound is 1e-10 px, not bit parity, fused multiply-adds only
# tighten the sums, and the pass is bound by float64 vector instructions, which contraction cuts by a quarter
# subpixel.hip: the float64 sub-pixel rule, compared bit for bit with tests/subpixel_oracle.py
# behaviour_segment.hip: the grid coordinates, the cell of a frame and the peak threshold are the operations of
# tests/behaviour_segment_oracle.py one by one: the integer outputs are compared exactly, and the density's bar assumes the oracle's coordinates
# gait.hip: the tip and its velocity are the subtractions, products and sums of tests/gait_oracle.py one by one: the
# velocity's bar counts those roundings, and the swing/stance thresholds then compare the number the bar was derived for
# pose_repair.hip: the deviation, the threshold, the score and the interpolated value are the operations of
# tests/pose_repair_oracle.py one by one, compared bit for bit
# treadmill.hip: the body-frame tips, their velocities and the slice sums of the sphere fit are the operations of
# tests/treadmill_oracle.py one by one, compared bit for bit; the bars of the solved quantities count those roundings
# track.hip: the unary and pair costs of the tracking model are the float64 operations of tests/track_oracle.py one
# by one, rounded once to int64; everything after that is integer arithmetic, compared exactly
# consensus.hip: the projection, the error and the sum of squares of the consensus model are the operations of
# tests/consensus_oracle.py one by one: the choice, the errors and the replaced detections are compared exactly on the device's own points
# trajectory.hip: the projection, the weights, H, g and the cost terms of the trajectory model are the operations of
# tests/trajectory_oracle.py one by one, compared bit for bit
# heatmap3d.hip: the projection, the Catmull-Rom weights, the taps' sums and the score of the heat-map triangulation are
# the operations of tests/heatmap3d_oracle.py one by one: the arg-max of a level is compared exactly wherever the oracle's two best scores
# lie further apart than the logarithm's rounding
# sync.hip: the Sampson distance of the camera-lag model is the float64 operations of tests/sync_oracle.py one by
# one, rounded once to int64; everything after that is integer arithmetic, compared exactly
# preprocess.hip and hourglass.hip, the two users of csrc/preprocess_math.h: the front-end's per-pixel arithmetic carries
# `#pragma clang fp contract(off)` so that (v / 255 - mean) / std and the bilinear taps round like the numpy statement, and an explicit
# -ffp-contract=fast DISREGARDS that pragma (the compiler fused v * (1 / 255) - mean and the taps).  fast-honor-pragmas, hipcc's own
# default, is `fast` everywhere else: of hourglass.hip's 158 kernels only the three stems' u8 sampling compiles differently
# (tests/test_gpu_frontend_sweep.py compares the identity size with the numpy expression bit for bit)
FILE_FLAGS = {"pose3d.hip": ["-ffp-contract=off"], "ba_lsmr.hip": ["-ffp-contract=off"], "render.hip": ["-ffp-contract=off"],
              "subpixel.hip": ["-ffp-contract=off"], "behaviour_segment.hip": ["-ffp-contract=off"], "gait.hip": ["-ffp-contract=off"],
              "pose_repair.hip": ["-ffp-contract=off"], "treadmill.hip": ["-ffp-contract=off"], "track.hip": ["-ffp-contract=off"],
              "consensus.hip": ["-ffp-contract=off"], "trajectory.hip": ["-ffp-contract=off"], "heatmap3d.hip": ["-ffp-contract=off"],
              "sync.hip": ["-ffp-contract=off"],
              "preprocess.hip": ["-ffp-contract=fast-honor-pragmas"], "hourglass.hip": ["-ffp-contract=fast-honor-pragmas"]}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain is required to build libdf3d_hip.so)")


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _digest(paths):
    h = hashlib.sha256()
    for p in sorted(paths):
        with open(p, "rb") as f:
            h.update(p.encode())
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def _deps():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(HERE, "..", "include", "df3d_hip.h"))
    return hdrs


def build(force=False, verbose=False):
    srcs = _sources()
    os.makedirs(OBJ_DIR, exist_ok=True)
    stamp = os.path.join(OBJ_DIR, "stamp")
    hdr_digest = _digest(_deps())
    hipcc = _hipcc()

    def compile_one(src):
        obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
        extra = FILE_FLAGS.get(os.path.basename(src), [])
        dig = _digest([src]) + hdr_digest + " ".join(extra)
        dig_file = obj + ".sha"
        if not force and os.path.exists(obj) and os.path.exists(dig_file) and open(dig_file).read() == dig:
            return obj, False
        cmd = [hipcc, *FLAGS, *extra, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr)
        with open(dig_file, "w") as f:
            f.write(dig)
        return obj, True

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        results = list(ex.map(compile_one, srcs))
    objs = [o for o, _ in results]
    changed = any(c for _, c in results)
    if changed or force or not os.path.exists(LIB_PATH):
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB_PATH, *objs]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        with open(stamp, "w") as f:
            f.write("ok")
    return LIB_PATH


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args()
    print(build(force=a.force, verbose=a.verbose))
