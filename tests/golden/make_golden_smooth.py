#!/usr/bin/env python3
"""Golden vectors for the manual half of the correction workflow, produced by *importing and executing* the
reference's own modules (df3d.signal_util, df3d.skeleton_fly) in the build container:

    python tests/golden/make_golden_smooth.py

Outputs (pure data):
  smooth_golden.npz     seeded [T, 38, 2] inputs `inp_T`, `smooth_pose2d` outputs `out_T` and `std_T`, the values np.std returned to
                        the reference's loop while it ran (recorded by wrapping np.std: one per frame, joint and coordinate), for
                        T in {1, 2, 9, 21, 400}.  The 400-frame case is a random walk (step sigma 1.5 px) around uniform offsets in
                        50 .. 900 px with sigma = 12 px noise added on frames 100-159 (both branches of the deviation test), joint 5
                        all zero and joint 23 zero on frames 200-259 (the "unseen" pattern).
  skeleton_tables.npz   camera_see_joint as bool [7, 38], ignore_joint_id.
  oneeuro2d_random.npz  filter_batch_2d on a 300-frame seeded walk.
Nothing at test/bench time reads /root/reference.
"""
import os
import sys

import numpy as np

REF = os.environ.get("DF3D_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 2, 9, 21, 400)


class RecordStd:
    """While active, every value np.std returns is kept: the reference calls it once per (frame, joint, coordinate), in that order."""

    def __enter__(self):
        self.values, self._std = [], np.std

        def recording(*args, **kw):
            self.values.append(self._std(*args, **kw))
            return self.values[-1]

        np.std = recording
        return self

    def __exit__(self, *exc):
        np.std = self._std


def main():
    sys.path.insert(0, REF)
    from df3d import skeleton_fly
    from df3d.signal_util import filter_batch_2d, smooth_pose2d

    rng = np.random.default_rng(20261016)
    data = {}
    for T in LENGTHS:
        walk = rng.uniform(50.0, 900.0, size=(1, 38, 2)) + np.cumsum(rng.normal(0.0, 1.5, size=(T, 38, 2)), axis=0)
        if T == 400:
            walk[100:160] += rng.normal(0.0, 12.0, size=(60, 38, 2))
            walk[:, 5] = 0.0
            walk[200:260, 23] = 0.0
        data[f"inp_{T}"] = walk
        with RecordStd() as seen:
            data[f"out_{T}"] = smooth_pose2d(np.copy(walk))
        data[f"std_{T}"] = np.array(seen.values, dtype=np.float64).reshape(walk.shape)
    np.savez(os.path.join(OUT, "smooth_golden.npz"), lengths=np.array(LENGTHS), **data)

    see = np.array([[bool(skeleton_fly.camera_see_joint(c, j)) for j in range(skeleton_fly.num_joints)] for c in range(7)])
    np.savez(os.path.join(OUT, "skeleton_tables.npz"), camera_see_joint=see, ignore_joint_id=np.array(skeleton_fly.ignore_joint_id, dtype=np.int64))

    walk = rng.uniform(50.0, 900.0, size=(1, 38, 2)) + np.cumsum(rng.normal(0.0, 1.5, size=(300, 38, 2)), axis=0)
    walk[100:103] += 60.0  # a jump, so the adaptive cut-off is exercised
    np.savez(os.path.join(OUT, "oneeuro2d_random.npz"), inp=walk, out=filter_batch_2d(np.copy(walk)))
    print("written")


if __name__ == "__main__":
    main()
