"""`df3d-cli` on the MI355X back-end: same flags, defaults and exit codes as reference df3d/cli.py:15-358.
Video rendering flags are accepted and reported as unsupported (visualisation is out of scope)."""
import argparse
import glob
import logging
import math
import os
import sys
from collections import deque
from pathlib import Path

from . import logger
from .core import Core
from .os_util import camera_videos


def parse_cli_args(argv=None):
    p = argparse.ArgumentParser(description="DeepFly3D pose estimation (MI355X back-end)")
    p.add_argument("-v", "--verbose", help="Enable info output (such as progress bars)", action="store_true")
    p.add_argument("-vv", "--verbose2", help="Enable debug output", action="store_true")
    p.add_argument("-d", "--debug", help="Displays the argument list for debugging purposes", action="store_true")
    p.add_argument("input_folder", help="Without additional arguments, a folder containing unlabeled images.", metavar="INPUT")
    p.add_argument("--output-folder", default=None,
                   help="Folder where results are written; default: INPUT suffixed with '_df3d'.")
    p.add_argument("-r", "--recursive", help="INPUT is a folder. Successively use its subfolders named 'images/'", action="store_true")
    p.add_argument("-f", "--from-file", help="INPUT is a text-file, where each line names a folder.", action="store_true")
    p.add_argument("-x", "--delete-images", help="Delete expanded image files after running (only if the .mp4 exists).", action="store_true")
    p.add_argument("-n", "--num-images-max", help="Maximal number of images to process (0 = all).", default=0, type=int)
    p.add_argument("--order", "--camera-ids", help="Ordering of the cameras, e.g. --order 0 1 4 3 2 5 6.",
                   default=[0, 1, 2, 3, 4, 5, 6], type=int, nargs="*")
    p.add_argument("--video-2d", help="Generate pose2d videos", action="store_true")
    p.add_argument("--video-3d", help="Generate pose3d videos", action="store_true")
    p.add_argument("--video-heatmap", dest="video_heatmap", action="store_true",
                   help="Generate a video of the 2 x 3 camera grid with the network's heat-maps drawn on the images: every pixel tinted with "
                        "the colour of the joint whose heat-map is largest there.  Needs only the images and the weights, so it also works "
                        "with --skip-pose-estimation")
    p.add_argument("--smooth-2d", dest="smooth_2d", action="store_true",
                   help="With --video-2d: draw the temporally smoothed 2-D detections (a 20-frame Gaussian where the detections are "
                        "quiet, the detection itself where they move) instead of the raw ones; results on disk are unchanged")
    p.add_argument("--video-quality", dest="video_quality", type=int, default=90, metavar="Q",
                   help="JPEG quality of the video frames, 1 .. 100 (default 90).  Has effect on the Motion-JPEG path only: the .avi written "
                        "when ffmpeg is not on PATH, whose frames are encoded on the GPU")
    p.add_argument("--skip-pose-estimation", help="Skip 2D and 3D pose estimation", dest="skip_estimation", action="store_true")
    p.add_argument("--batch-size", help="Batch size for inference", type=int, default=8)
    p.add_argument("--pin-memory-disabled", help="Disable pinned host staging buffers", action="store_true")
    p.add_argument("--output-fps", help="FPS for output videos.", type=float, default=None)
    p.add_argument("--dtype", choices=["f32", "f32s", "f16", "bf16"], default="f32",
                   help="hourglass arithmetic on the GPU: f32 (default: the reference's arithmetic); f32s = float32 tensors, weights and accumulation with "
                        "every product formed from IEEE-half splits on the 16-bit matrix cores, ~2.2x faster, heat-maps ~2e-6 of their range from f32's "
                        "(MEASURED on seeded synthetic weights; operands must lie inside the half range 65 504, which batch-normalised activations do); f16 = IEEE-half activations and weights on the "
                        "matrix cores with fp32 accumulation, ~6x faster; MEASURED on seeded synthetic weights against the fp32 oracle: heat-map confidences "
                        "6-8e-4 off on peaked maps, up to 2.8e-3 on flat ones (the reference's test tolerance is 2e-3, tests/test_df3d.py:173-178; "
                        "with the trained checkpoint unverified: tests/test_gpu_reference_pin.py decides once weights are present); bf16 = same speed, "
                        "fp32's exponent range, 8 significant bits: confidences ~6e-3 off on peaked maps, outside that tolerance.  f16 / f32s refuse weights beyond "
                        "the half range when they are loaded, and if an activation overflows on real images (an infinity or a NaN in any heat-map) the run "
                        "stops with an error that says so instead of writing df3d_result.pkl: rerun with --dtype f32")
    p.add_argument("--auto-correct", dest="auto_correct", action="store_true",
                   help="Correct the 2-D detections with the pictorial-structures model (bone-length prior, multi-view reprojection "
                        "consistency over the heat-map peaks) before triangulating; the arg-max detections are kept as points2d_argmax")
    p.add_argument("--correct-only-flagged", dest="correct_only_flagged", action="store_true",
                   help="With --auto-correct: keep the correction only on the joints whose reprojection error exceeds the per-joint "
                        "threshold (40 px) on the arg-max detections; every other detection stays the arg-max one")
    p.add_argument("--track-2d", dest="track_2d", action="store_true",
                   help="Track the 2-D detections through time before the first save: for every camera and network joint, the sequence of "
                        "heat-map peaks that is jointly best over the whole recording (an exact Viterbi solve: a peak pays for the heat-map "
                        "value it gives up against the frame's best and for its jump from the frame before) replaces the per-frame arg-max; "
                        "the arg-max detections are kept as points2d_argmax, followed by track_choice [7, T, 19], track_cost [7, 19] and "
                        "track_params.  --track-tau and the two weights are guesses that nobody has measured on a recording.  Not together "
                        "with --auto-correct or --skip-pose-estimation")
    p.add_argument("--track-tau", dest="track_tau", type=float, default=None, metavar="PX",
                   help="With --track-2d: the jump between consecutive frames, in pixels, beyond which every jump costs the same (default 30)")
    p.add_argument("--track-motion", dest="track_motion", type=float, default=None, metavar="W",
                   help="With --track-2d: the weight of the jump term, 0 to 1024 (default 1); 0 leaves every detection the arg-max")
    p.add_argument("--track-value", dest="track_value", type=float, default=None, metavar="W",
                   help="With --track-2d: the weight of the heat-map value term, 0 to 1024 (default 1)")
    p.add_argument("--subpixel", action="store_true",
                   help="Refine every 2-D detection inside its heat-map cell (up to half a cell, 3.75 px, per axis) from the 3 x 3 values round the "
                        "maximum instead of reporting the cell itself; the result then carries the key subpixel.  Off by default: the default is the "
                        "reference's arithmetic")
    p.add_argument("--joint-angles", dest="joint_angles", action="store_true",
                   help="Append the leg joint angles (8 per leg, radians) and segment lengths (4 per leg) of the triangulated pose to the "
                        "result, as the keys joint_angles [T, 6, 8] and segment_lengths [T, 6, 4]; the body frame is the recording's, from "
                        "the temporal medians of the six body-coxa joints.  Works with --skip-pose-estimation on an earlier result")
    p.add_argument("--rigid-legs", dest="rigid_legs", action="store_true",
                   help="Fit legs of constant segment lengths (each segment's median over the recording) to the triangulated pose and append "
                        "the keys points3d_rigid [T, 38, 3], rigid_segment_lengths [6, 4] and rigid_fit_cost [T, 6] to the result; together "
                        "with --joint-angles also joint_angles_rigid [T, 6, 8], the angles of the fitted pose.  Works with "
                        "--skip-pose-estimation on an earlier result")
    p.add_argument("--angle-spectrogram", dest="angle_spectrogram", action="store_true",
                   help="Append the Morlet wavelet amplitudes of the 48 joint-angle series to the result, as the keys angle_spectrogram "
                        "[T, 6, 8, F] (float32, radians), spectrogram_freqs [F] (Hz) and spectrogram_fps: 25 frequencies from 1 Hz to a quarter "
                        "of the frame rate (100 fps where the recording has no videos to read it from); together with --rigid-legs also "
                        "angle_spectrogram_rigid, the same of the fitted pose.  The angles themselves are stored only with --joint-angles.  "
                        "Works with --skip-pose-estimation on an earlier result")
    p.add_argument("--behaviour-map", dest="behaviour_map", action="store_true",
                   help="Embed every frame's joint-angle spectrogram (the one --angle-spectrogram computes, normalised per frame) in the plane "
                        "by t-SNE under the Kullback-Leibler divergence and append the keys behaviour_map [T, 2] (float64; NaN for a frame "
                        "without a spectrum), behaviour_map_train_index, behaviour_map_kl and behaviour_map_perplexity to the result; together "
                        "with --rigid-legs also behaviour_map_rigid and behaviour_map_rigid_kl.  The spectrogram itself is stored only with "
                        "--angle-spectrogram.  Works with --skip-pose-estimation on an earlier result")
    p.add_argument("--behaviour-perplexity", dest="behaviour_perplexity", type=float, default=None, metavar="U",
                   help="With --behaviour-map: the effective number of neighbours of a frame (default 32).  The recording needs at least "
                        "3 U + 1 frames")
    p.add_argument("--behaviour-segments", dest="behaviour_segments", action="store_true",
                   help="With --behaviour-map: segment the map and append the keys behaviour_density [G, G] (the Gaussian density of the frames on "
                        "a square grid), behaviour_density_origin (x0, y0 and the cell size h), behaviour_density_sigma, behaviour_regions [G, G] (the "
                        "watershed region of every cell round the density's peaks, 0: none), behaviour_region_peaks [R, 2], behaviour_labels [T] "
                        "(int32: every frame's region, 0: none, -1: a frame without a place on the map), behaviour_bouts [B, 3] (label, start, "
                        "length), behaviour_occupancy and behaviour_transitions to the result; together with --rigid-legs also the same nine "
                        "with _rigid appended.  Works with --skip-pose-estimation on an earlier result")
    p.add_argument("--behaviour-sigma", dest="behaviour_sigma", type=float, default=None, metavar="S",
                   help="With --behaviour-segments: the deviation of the density's Gaussians in the map's units (default 1/32 of the map's extent)")
    p.add_argument("--behaviour-grid", dest="behaviour_grid", type=int, default=None, metavar="G",
                   help="With --behaviour-segments: the cells per side of the density's grid, 2 to 1024 (default 256)")
    p.add_argument("--gait", dest="gait", action="store_true",
                   help="Analyse the gait from the leg tips and append, after every other key, gait_tip_position and gait_tip_velocity [T, 6, 3] "
                        "(every tip relative to its body-coxa joint and its velocity, in leg coordinates), gait_states [T, 6] (int8: -1 unknown, "
                        "0 stance, 1 swing, by hysteresis on the tip's anterior velocity), gait_steps [S, 4] (leg, lift-off, touch-down, next "
                        "lift-off), gait_step_metrics [S, 3] (swing duration, stance duration, stride), gait_phase [T, 6], gait_coupling [6, 6, 2] "
                        "and gait_coupling_count [6, 6], gait_pattern [T] (the mask of the legs in swing; 21 and 42 are the tripods), "
                        "gait_pattern_histogram [64], gait_state_counts [6, 3], gait_thresholds and gait_fps to the result; together with "
                        "--rigid-legs also the same thirteen with _rigid appended.  Works with --skip-pose-estimation on an earlier result")
    p.add_argument("--gait-on", dest="gait_on", type=float, default=None, metavar="V",
                   help="With --gait: the anterior tip velocity above which a leg goes into swing, in pose units (mm) per second (default 5, a "
                        "guess from published tip speeds that nobody has measured on a recording)")
    p.add_argument("--gait-off", dest="gait_off", type=float, default=None, metavar="V",
                   help="With --gait: the anterior tip velocity below which a leg goes into stance (default 0, a guess like --gait-on); it must "
                        "lie below --gait-on")
    p.add_argument("--treadmill", dest="treadmill", action="store_true",
                   help="Estimate the treadmill ball and the fictive walking path from the leg tips in stance: one sphere through the stance "
                        "tips, the ball's rotation in every frame from their velocities, and the path the fly would have walked.  Appends, "
                        "after the gait keys, treadmill_ball_center [3], treadmill_ball_radius, treadmill_ball_rms, treadmill_ball_count, "
                        "treadmill_ball_status (bit 0: the fit was refused), treadmill_rotation [T, 3] (rad/s), treadmill_legs [T], "
                        "treadmill_residual [T], treadmill_fictive [T, 3] (forward and sideways speed in mm/s, yaw rate in rad/s), "
                        "treadmill_path [T, 3] (x, y, heading), treadmill_skipped, treadmill_params and treadmill_fps to the result.  The "
                        "swing thresholds are --gait's defaults, guesses that nobody has measured on a recording; a spiked tip shows here "
                        "first, which --repair-pose is for.  Works with --skip-pose-estimation on an earlier result")
    p.add_argument("--ball-radius", dest="ball_radius", type=float, default=None, metavar="MM",
                   help="With --treadmill: the ball's known radius in pose units (mm); without it the radius is fitted, and noise on the "
                        "tips biases the fitted radius low")
    p.add_argument("--repair-pose", dest="repair_pose", action="store_true",
                   help="Repair the triangulated pose before the kinematics: a joint that lies further from the median of the frames round it "
                        "than --repair-threshold robust deviations (a Hampel test, per coordinate, one pass) is an outlier; outliers and missing "
                        "joints are interpolated linearly over gaps of at most --repair-max-gap frames and set to 0 (missing) otherwise.  "
                        "Appends, after every other key, points3d_repaired [T, 38, 3], repair_status [T, 38] (int8: 0 kept, 1 missing and "
                        "filled, 2 outlier and filled, 3 missing and left, 4 outlier and removed), repair_counts [38, 5], repair_score [T, 38] "
                        "and repair_params to the result, and every other opt-in key (--joint-angles, --rigid-legs, --angle-spectrogram, "
                        "--behaviour-map, --gait) is computed from the repaired pose; points3d and points3d_wo_procrustes stay the "
                        "triangulation's own.  The defaults are guesses that nobody has measured on a recording, and a test on positions is "
                        "blind to a spike smaller than the threshold times the local spread of a fast-moving tip.  Works with "
                        "--skip-pose-estimation on an earlier result")
    p.add_argument("--repair-window", dest="repair_window", type=int, default=None, metavar="H",
                   help="With --repair-pose: the frames to either side of a frame that its median is taken over, 1 to 64 (default 5, a guess)")
    p.add_argument("--repair-threshold", dest="repair_threshold", type=float, default=None, metavar="K",
                   help="With --repair-pose: the robust deviations (1.4826 times the window's median absolute deviation) beyond which a joint is "
                        "an outlier (default 6, a guess)")
    p.add_argument("--repair-floor", dest="repair_floor", type=float, default=None, metavar="MM",
                   help="With --repair-pose: the deviation, in pose units (mm), below which a joint is never an outlier (default 0.05, a guess)")
    p.add_argument("--repair-max-gap", dest="repair_max_gap", type=int, default=None, metavar="N",
                   help="With --repair-pose: the longest run of bad frames of a joint that is interpolated, 0 to 1000000 (default 10, a guess)")
    p.add_argument("--robust-triangulation", dest="robust_triangulation", action="store_true",
                   help="Triangulate every joint from the largest set of cameras that agree: every subset of the cameras that see a joint is "
                        "triangulated, a subset qualifies when each of its cameras reprojects its point within --robust-tau pixels, and the "
                        "largest qualifying subset wins (ties to the smaller squared error).  Appends, after every other key, "
                        "points3d_robust [T, 38, 3], robust_cameras [T, 38] (bit c: camera c was used), robust_status [T, 38] (int8: 0 fewer "
                        "than two views, 1 all views agree, 2 a subset was chosen, 3 none qualified: the plain triangulation), robust_error "
                        "[7, T, 38], robust_counts [38, 4], points2d_robust [7, T, 38, 2] (rejected detections replaced by the projection) "
                        "and robust_params to the result, and every other opt-in key is computed from the robust pose (repaired afterwards "
                        "with --repair-pose); points3d, points3d_wo_procrustes and points2d stay the plain triangulation's.  Two views that "
                        "agree with each other cannot be told from two correct ones: with three views a wrong detection near an epipolar "
                        "line wins.  The default threshold is a guess that nobody has measured on a recording.  Works with "
                        "--skip-pose-estimation on an earlier result")
    p.add_argument("--robust-tau", dest="robust_tau", type=float, default=None, metavar="PX",
                   help="With --robust-triangulation: the reprojection error, in pixels, within which a camera agrees with a subset's point "
                        "(default 20, a guess)")
    p.add_argument("--robust-min-views", dest="robust_min_views", type=int, default=None, metavar="N",
                   help="With --robust-triangulation: the fewest cameras a subset may hold, 2 to 8 (default 2)")
    p.add_argument("--ba-loss", dest="ba_loss", choices=("linear", "soft_l1", "huber", "cauchy", "arctan"), default=None,
                   help="The loss of the calibration's bundle adjustment on the reprojection residuals, with the meaning of scipy's "
                        "least_squares(loss=): linear (the default) is the plain sum of squares, which believes every detection; with the "
                        "others a wrong detection stops pulling the cameras.  soft_l1 is the one to use: huber and cauchy can stall at the "
                        "start.  Appends, after every other key, ba_weight [7, T, 38] (1: the detection counted in full, NaN: it was not "
                        "in the adjustment), ba_counts [7, 3] and ba_params to the result.  On a joint that two cameras see, a wrong "
                        "detection cannot be told from a wrong point: the loss only bounds its pull")
    p.add_argument("--ba-f-scale", dest="ba_f_scale", type=float, default=None, metavar="PX",
                   help="With --ba-loss: the residual, in pixels, up to which a detection counts in full (default 4: about two standard "
                        "deviations of a 7.5 px heat-map cell's quantisation -- a guess that nobody has measured on a recording)")
    p.add_argument("--trajectory-triangulation", dest="trajectory_triangulation", action="store_true",
                   help="Fit every joint's 3-D trajectory to the 2-D detections of the whole recording: per joint the points minimise a Huber "
                        "loss (--trajectory-huber pixels) of every camera's reprojection error plus --trajectory-lambda times the squared "
                        "second differences of the trajectory.  A frame one camera sees is fitted to that view and its neighbours instead "
                        "of being written as missing, a detection that jumps away from the trajectory is down-weighted, and depth along a "
                        "ray is smoothed more than the directions across it.  Appends, after every other key, points3d_trajectory "
                        "[T, 38, 3], trajectory_status [T, 38] (int8: 0 outside every segment, the plain triangulation; 1 fitted; 2 filled "
                        "from fewer than two views; 3 filled without a view; 4 the joint's fit did not converge), trajectory_weight "
                        "[7, T, 38] (below 1: the camera to correct), trajectory_error [7, T, 38], trajectory_iterations [38], "
                        "trajectory_cost [38, 2], trajectory_counts [38, 5] and trajectory_params to the result, and every other opt-in "
                        "key is computed from the trajectory pose (repaired afterwards with --repair-pose); with --robust-triangulation "
                        "the fit starts from the robust points and uses only the views the consensus kept.  points3d, "
                        "points3d_wo_procrustes and points2d stay the plain triangulation's.  On clean detections the gain over the plain "
                        "triangulation is small.  The defaults are guesses that nobody has measured on a recording.  Works with "
                        "--skip-pose-estimation on an earlier result")
    p.add_argument("--trajectory-lambda", dest="trajectory_lambda", type=float, default=None, metavar="L",
                   help="With --trajectory-triangulation: the weight of the smoothness term, in px^2 / mm^2, >= 0 (default 1e3, a guess; 0 "
                        "decouples the frames)")
    p.add_argument("--trajectory-huber", dest="trajectory_huber", type=float, default=None, metavar="PX",
                   help="With --trajectory-triangulation: the reprojection error, in pixels, beyond which a view's loss grows linearly "
                        "(default 10, a guess; inf is plain least squares)")
    p.add_argument("--trajectory-max-gap", dest="trajectory_max_gap", type=int, default=None, metavar="N",
                   help="With --trajectory-triangulation: the longest run of frames without two views that a segment bridges, 0 to 1000000 "
                        "(default 10, a guess)")
    p.add_argument("--heatmap-triangulation", dest="heatmap_triangulation", action="store_true",
                   help="Search every joint's 3-D point on the heat-maps themselves: the point is where the product of the heat-maps of the "
                        "cameras that see the joint, each read at the point's projection, is largest -- a coarse-to-fine search over 8 x 8 x 8 "
                        "points round the latest pose (--heatmap-levels times, the first cube --heatmap-half mm to either side).  It uses a "
                        "second peak or an elongated blob that the arg-max throws away: decisive where a heat-map has two peaks and three "
                        "cameras see the joint, 1.5 to 2 times better on elongated blobs, nothing to slightly worse than --subpixel on clean "
                        "round ones, and not measured on trained weights.  With two cameras two peaks in one view cannot be told apart.  "
                        "Appends, after every other key, points3d_heatmap [T, 38, 3], heatmap3d_status [T, 38] (int8: 0 fewer than two "
                        "views or no start point, 1 searched, 2 no evidence within the cube, 3 searched and the best point of the first "
                        "level lay on a face of the cube), heatmap3d_score, heatmap3d_views, heatmap3d_shift [T, 38], heatmap3d_counts "
                        "[38, 4] and heatmap3d_params to the result, and every other opt-in key is computed from this pose (repaired "
                        "afterwards with --repair-pose); it runs after --robust-triangulation and --trajectory-triangulation and starts "
                        "from their pose.  points3d, points3d_wo_procrustes and points2d stay the plain triangulation's.  The heat-maps are "
                        "recomputed from the images (a second pass of the network), never stored: the images must be present.  The "
                        "defaults are guesses that nobody has measured on a recording.  Works with --skip-pose-estimation on an earlier "
                        "result while the images are present")
    p.add_argument("--heatmap-half", dest="heatmap_half", type=float, default=None, metavar="MM",
                   help="With --heatmap-triangulation: the half width of the first cube, in pose units (mm), > 0 (default 0.4, a guess)")
    p.add_argument("--heatmap-levels", dest="heatmap_levels", type=int, default=None, metavar="N",
                   help="With --heatmap-triangulation: the levels of the search, 1 to 6 (default 4: a last step of 0.0016 mm); each level "
                        "divides the step by 4")
    p.add_argument("--heatmap-floor", dest="heatmap_floor", type=float, default=None, metavar="E",
                   help="With --heatmap-triangulation: the heat-map value at and below which a cell says nothing, between 0 and 1 "
                        "(default 1e-3, a guess)")
    p.add_argument("--check-sync", dest="check_sync", action="store_true",
                   help="Check that frame t of every camera shows the same instant: for every pair of cameras that see a common joint, the "
                        "detections of one camera are compared with the other's up to --sync-max-lag frames earlier and later, by their "
                        "distance to the pair's epipolar lines, per window of --sync-window frames; a camera that dropped a frame shows "
                        "up as a lag from that window on.  Needs only the detections and the calibration.  Appends, after every other "
                        "key, sync_lag [7, nW] (camera c shows instant t in its frame t + lag), sync_status [7] (0 the camera shares no "
                        "joint with another, 1 in step, 2 lagging somewhere), sync_pairs, sync_pair_lag, sync_pair_margin, "
                        "sync_pair_inconsistency, sync_pair_cost, sync_pair_count and sync_params to the result, and logs one line per "
                        "lagging camera.  Lags are relative within a group of cameras that share joints: a lag between the left and the "
                        "right cameras cannot be seen.  The defaults are guesses that nobody has measured on a recording.  Works with "
                        "--skip-pose-estimation on an earlier result")
    p.add_argument("--sync-cameras", dest="sync_cameras", action="store_true",
                   help="--check-sync, and undo the lags before triangulating: camera c's detection of instant t is taken from its frame "
                        "t + lag (unseen where that frame does not exist); points2d and every later stage of the save hold the shifted "
                        "detections, and the originals are kept as points2d_unsynced.  Not with --auto-correct, --track-2d, "
                        "--heatmap-triangulation or --video-heatmap, which read heat-maps by frame index")
    p.add_argument("--sync-max-lag", dest="sync_max_lag", type=int, default=None, metavar="N",
                   help="With --check-sync or --sync-cameras: the largest lag searched, in frames, 0 to 64 (default 8)")
    p.add_argument("--sync-window", dest="sync_window", type=int, default=None, metavar="W",
                   help="With --check-sync or --sync-cameras: the frames of a window, >= 1 (default 256): a lag is constant inside one")
    p.add_argument("--sync-tau", dest="sync_tau", type=float, default=None, metavar="PX",
                   help="With --check-sync or --sync-cameras: the epipolar distance, in pixels, at which a sample's cost is truncated "
                        "(default 20, a guess)")
    p.add_argument("--sync-switch", dest="sync_switch", type=float, default=None, metavar="K",
                   help="With --check-sync or --sync-cameras: the cost, in px^2 per frame of lag, of changing the lag between neighbouring "
                        "windows (default 64, a guess): a window without motion then keeps its neighbours' lag")
    args = p.parse_args(argv)
    for name in ("max_lag", "window", "tau", "switch"):
        if getattr(args, "sync_" + name) is not None and not (args.check_sync or args.sync_cameras):
            p.error(f"--sync-{name.replace('_', '-')} sets a parameter of --check-sync and --sync-cameras: it needs one of them")
    if args.check_sync or args.sync_cameras:
        from . import sync

        try:
            sync.sync_params(args.sync_max_lag, args.sync_window, args.sync_tau, args.sync_switch)
        except ValueError as e:
            p.error(f"--sync-max-lag, --sync-window, --sync-tau and --sync-switch: {e}")
    if args.sync_cameras:
        for flag in ("auto_correct", "track_2d", "heatmap_triangulation", "video_heatmap"):
            if getattr(args, flag, False):
                p.error(f"--sync-cameras shifts the detections' frames, and --{flag.replace('_', '-')} reads the heat-maps by frame index: "
                        "they cannot be combined")
    for name in ("half", "levels", "floor"):
        if getattr(args, "heatmap_" + name) is not None and not args.heatmap_triangulation:
            p.error(f"--heatmap-{name} sets a parameter of --heatmap-triangulation: it needs --heatmap-triangulation")
    if args.heatmap_triangulation:
        from . import heatmap3d

        try:
            heatmap3d.heatmap3d_params(args.heatmap_half, args.heatmap_levels, args.heatmap_floor)
        except ValueError as e:
            p.error(f"--heatmap-half, --heatmap-levels and --heatmap-floor: {e}")
    for name in ("lambda", "huber", "max_gap"):
        if getattr(args, "trajectory_" + name) is not None and not args.trajectory_triangulation:
            p.error(f"--trajectory-{name.replace('_', '-')} sets a parameter of --trajectory-triangulation: it needs --trajectory-triangulation")
    if args.trajectory_triangulation:
        from . import ops

        try:
            ops.trajectory_params(args.trajectory_lambda, args.trajectory_huber, args.trajectory_max_gap)
        except ValueError as e:
            p.error(f"--trajectory-lambda, --trajectory-huber and --trajectory-max-gap: {e}")
    if args.ba_f_scale is not None:
        if args.ba_loss in (None, "linear"):
            p.error("--ba-f-scale sets a parameter of --ba-loss: it needs --ba-loss with a loss other than linear")
        if not (args.ba_f_scale > 0 and args.ba_f_scale != float("inf")):
            p.error("--ba-f-scale must be positive and finite")
    for name in ("tau", "min_views"):
        if getattr(args, "robust_" + name) is not None and not args.robust_triangulation:
            p.error(f"--robust-{name.replace('_', '-')} sets a parameter of --robust-triangulation: it needs --robust-triangulation")
    if args.robust_triangulation:
        from . import ops

        try:
            ops.consensus_params(args.robust_tau, args.robust_min_views)
        except ValueError as e:
            p.error(f"--robust-tau and --robust-min-views: {e}")
    for name in ("window", "threshold", "floor", "max_gap"):
        if getattr(args, "repair_" + name) is not None and not args.repair_pose:
            p.error(f"--repair-{name.replace('_', '-')} sets a parameter of --repair-pose: it needs --repair-pose")
    if args.repair_pose:
        from . import ops

        try:
            ops.repair_params(args.repair_window, args.repair_threshold, args.repair_floor, args.repair_max_gap)
        except ValueError as e:
            p.error(f"--repair-window, --repair-threshold, --repair-floor and --repair-max-gap: {e}")
    if args.ball_radius is not None and not args.treadmill:
        p.error("--ball-radius sets the radius of --treadmill: it needs --treadmill")
    if args.treadmill:
        from . import ops

        try:
            ops.treadmill_params(args.ball_radius)
        except ValueError as e:
            p.error(f"--ball-radius: {e}")
    if args.gait_on is not None and not args.gait:
        p.error("--gait-on sets the swing threshold of --gait: it needs --gait")
    if args.gait_off is not None and not args.gait:
        p.error("--gait-off sets the stance threshold of --gait: it needs --gait")
    if args.gait:
        from . import ops

        try:
            ops.gait_thresholds(args.gait_on, args.gait_off)
        except ValueError as e:
            p.error(f"--gait-on and --gait-off: {e}")
    if args.behaviour_segments and not args.behaviour_map:
        p.error("--behaviour-segments segments the map of --behaviour-map: it needs --behaviour-map")
    if args.behaviour_sigma is not None and not args.behaviour_segments:
        p.error("--behaviour-sigma sets the density of --behaviour-segments: it needs --behaviour-segments")
    if args.behaviour_grid is not None and not args.behaviour_segments:
        p.error("--behaviour-grid sets the grid of --behaviour-segments: it needs --behaviour-segments")
    if args.behaviour_sigma is not None and not (math.isfinite(args.behaviour_sigma) and args.behaviour_sigma > 0.0):
        p.error("--behaviour-sigma must be finite and > 0")
    if args.behaviour_grid is not None and not 2 <= args.behaviour_grid <= 1024:
        p.error("--behaviour-grid must be in [2, 1024]")
    if args.behaviour_perplexity is not None and not args.behaviour_map:
        p.error("--behaviour-perplexity sets the perplexity of --behaviour-map: it needs --behaviour-map")
    if args.behaviour_perplexity is not None and not (math.isfinite(args.behaviour_perplexity) and args.behaviour_perplexity > 1.0):
        p.error("--behaviour-perplexity must be finite and > 1")
    for name in ("tau", "motion", "value"):
        if getattr(args, "track_" + name) is not None and not args.track_2d:
            p.error(f"--track-{name} sets a parameter of --track-2d: it needs --track-2d")
    if args.track_2d:
        from . import ops

        if args.skip_estimation:
            p.error("--track-2d needs the heat-map peaks of this run's pose estimation: it cannot be combined with --skip-pose-estimation")
        if args.auto_correct:
            p.error("--track-2d and --auto-correct both start from the arg-max detections, so the later one would undo the other: choose one")
        try:
            ops.track_params(args.track_tau, args.track_motion, args.track_value)
        except ValueError as e:
            p.error(f"--track-tau, --track-motion and --track-value: {e}")
    if args.auto_correct and args.skip_estimation:
        p.error("--auto-correct needs the heat-map peaks of this run's pose estimation: it cannot be combined with --skip-pose-estimation")
    if args.subpixel and args.skip_estimation:
        p.error("--subpixel needs the heat-maps of this run's pose estimation: it cannot be combined with --skip-pose-estimation")
    if args.correct_only_flagged and not args.auto_correct:
        p.error("--correct-only-flagged restricts --auto-correct: it needs --auto-correct")
    if args.smooth_2d and not args.video_2d:
        p.error("--smooth-2d changes what --video-2d draws: it needs --video-2d")
    if not 1 <= args.video_quality <= 100:
        p.error(f"--video-quality is a JPEG quality, 1 .. 100: got {args.video_quality}")
    inp =Path(args.input_folder).expanduser().resolve()
    args.output_folder = str(inp.with_name(inp.stem + "_df3d")) if args.output_folder is None else str(Path(args.output_folder).expanduser().resolve())
    args.input_folder = str(inp)
    return args


def setup_logger(args):
    handler = logging.StreamHandler()
    handler.setLevel(logging.DEBUG)
    lg = logger.getLogger()
    lg.addHandler(handler)
    lg.setLevel(logging.DEBUG if args.verbose2 else logging.INFO if args.verbose else logging.WARNING)


def print_debug(args):
    print(f"Enabled logging level: {logging.getLevelName(logger.getLogger().getEffectiveLevel())}")
    print("Arguments are:")
    for k, v in vars(args).items():
        print(f"\t{k}: {v}")
    print()
    return 0


# heat-maps are never stored: once an earlier --delete-images has removed the frames, and they cannot be expanded again
# from the camera videos, there is nothing to compute them from
_NO_IMAGES = ("--video-heatmap draws the heat-maps the network computes from the camera images, and {folder} holds none (removed by an earlier "
              "--delete-images?): heat-maps are recomputed from the images, never stored, so there is nothing to draw")
_NO_IMAGES_3D = ("--heatmap-triangulation searches the heat-maps the network computes from the camera images, and {folder} holds none (removed by "
                 "an earlier --delete-images?): heat-maps are recomputed from the images, never stored, so there is nothing to search")


def run(args):
    video_heatmap = getattr(args, "video_heatmap", False)
    # what the second save appends to the result: the kinematics flags, in the order of their keys, and the map's perplexity
    extras = {name: getattr(args, name, False) for name in ("joint_angles", "rigid_legs", "angle_spectrogram", "behaviour_map", "gait", "treadmill",
                                                                "repair_pose")}
    flagged = [name for name, on in extras.items() if on]
    extras["behaviour_perplexity"] = getattr(args, "behaviour_perplexity", None)
    if getattr(args, "behaviour_segments", False):   # the map's segmentation: no keys of its own flag without --behaviour-map
        extras.update(behaviour_segments=True, behaviour_sigma=getattr(args, "behaviour_sigma", None), behaviour_grid=getattr(args, "behaviour_grid", None))
    if extras["gait"]:
        extras.update(gait_on=getattr(args, "gait_on", None), gait_off=getattr(args, "gait_off", None))
    if extras["treadmill"]:
        extras.update(ball_radius=getattr(args, "ball_radius", None))
    if extras["repair_pose"]:
        extras.update({name: getattr(args, name, None) for name in ("repair_window", "repair_threshold", "repair_floor", "repair_max_gap")})
    if getattr(args, "robust_triangulation", False):   # after the other flags: its keys come last
        flagged.append("robust_triangulation")
        extras.update(robust_triangulation=True, robust_tau=getattr(args, "robust_tau", None), robust_min_views=getattr(args, "robust_min_views", None))
    if getattr(args, "trajectory_triangulation", False):   # after the robust keys
        flagged.append("trajectory_triangulation")
        extras.update(trajectory_triangulation=True, trajectory_lambda=getattr(args, "trajectory_lambda", None),
                      trajectory_huber=getattr(args, "trajectory_huber", None), trajectory_max_gap=getattr(args, "trajectory_max_gap", None))
    heatmap3d = getattr(args, "heatmap_triangulation", False)
    if heatmap3d:   # after the trajectory keys
        flagged.append("heatmap_triangulation")
        extras.update(heatmap_triangulation=True, heatmap_half=getattr(args, "heatmap_half", None), heatmap_levels=getattr(args, "heatmap_levels", None),
                      heatmap_floor=getattr(args, "heatmap_floor", None))
    if getattr(args, "check_sync", False) or getattr(args, "sync_cameras", False):   # after the heat-map keys
        flagged.append("sync_cameras" if getattr(args, "sync_cameras", False) else "check_sync")
        extras.update(check_sync=True, sync_cameras=getattr(args, "sync_cameras", False), sync_max_lag=getattr(args, "sync_max_lag", None),
                      sync_window=getattr(args, "sync_window", None), sync_tau=getattr(args, "sync_tau", None),
                      sync_switch=getattr(args, "sync_switch", None))
    if args.skip_estimation and not args.video_2d and not args.video_3d and not video_heatmap and not flagged:
        logger.info("Nothing to do. Check your command-line arguments.")
        return 0
    logger.info(f"\nWorking in {args.input_folder}")
    if video_heatmap and not glob.glob(os.path.join(args.input_folder, "camera_*_img_*.jpg")) and not camera_videos(args.input_folder):
        raise FileNotFoundError(_NO_IMAGES.format(folder=args.input_folder))   # before Core: neither frames nor videos to expand them from
    core = Core(args.input_folder, args.output_folder, args.num_images_max, args.order, dtype=args.dtype, device=getattr(args, "device", None))
    if video_heatmap and not core.has_heatmap:
        raise FileNotFoundError(_NO_IMAGES.format(folder=args.input_folder))
    if heatmap3d and not core.has_heatmap:
        raise FileNotFoundError(_NO_IMAGES_3D.format(folder=args.input_folder))
    if flagged and args.skip_estimation and core.points2d is None:
        raise RuntimeError(f"--{flagged[0].replace('_', '-')} needs calibrated cameras to triangulate with, and with --skip-pose-estimation "
                           f"{args.output_folder} holds no earlier result to reopen: run the pose estimation first")
    if extras["behaviour_map"]:   # a recording too short for the perplexity: refused before any work
        from . import ops

        ops.behaviour_map_points(core.num_images, extras["behaviour_perplexity"])
    auto = getattr(args, "auto_correct", False)
    if not args.skip_estimation:
        from .config import PICTORIAL_DEFAULTS

        track = getattr(args, "track_2d", False)
        core.pose2d_estimation(args.batch_size, args.pin_memory_disabled, num_peaks=PICTORIAL_DEFAULTS["num_peaks"] if auto or track else 0,
                               subpixel=getattr(args, "subpixel", False))
        if track:   # before the first save: the calibration then starts from the tracked detections
            given = {"tau": getattr(args, "track_tau", None), "w_motion": getattr(args, "track_motion", None),
                     "w_value": getattr(args, "track_value", None)}
            core.track_detections(**{name: v for name, v in given.items() if v is not None})
        core.save()
    # the heat-map video needs the images and the weights only: without an earlier result to reopen there is no pose to calibrate or save
    pose_free = args.skip_estimation and core.points2d is None and video_heatmap and not args.video_2d and not args.video_3d
    if not pose_free:
        core.calibrate_calc(0, core.max_img_id, loss=getattr(args, "ba_loss", None), f_scale=getattr(args, "ba_f_scale", None))
        if auto and getattr(args, "correct_only_flagged", False):
            core.auto_correct(flagged_only=True)
        elif auto:
            core.auto_correct()
        core.save(**extras)
    if args.video_2d or args.video_3d or video_heatmap:
        # f4 (reference cli.py:305-321): frames drawn on the GPU (csrc/render.hip), encoded by ffmpeg when present.  Rank 0 draws and
        # encodes; the peers wait for its outcome with a heartbeat (distributed.primary_section), so that an encoder failure moves
        # every rank on to the next folder together and a long encode never holds a peer in one collective
        from . import distributed as dd
        from . import video

        fps = args.output_fps if args.output_fps is not None else core.fps

        quality = getattr(args, "video_quality", 90)

        def videos(beat):
            if args.video_2d:
                video.make_pose2d_video(core, fps=fps, progress=beat, smooth=getattr(args, "smooth_2d", False), quality=quality)
            if args.video_3d:
                video.make_pose3d_video(core, fps=fps, progress=beat, quality=quality)
            if video_heatmap:
                video.make_heatmap_video(core, fps=fps, progress=beat, quality=quality)

        dd.primary_section(videos, "video")
    if args.delete_images:
        core.delete_images()
    return 0


def run_in_folders(args, folders):
    errors = []
    for folder in folders:
        try:
            args.input_folder = str(folder)  # like the reference, every folder writes into the one output folder
            run(args)
        except KeyboardInterrupt:
            logger.warning("Keyboard Interrupt received. Terminating...")
            break
        except Exception as e:  # per-folder isolation, as the reference does
            errors.append((folder, e))
            logger.error(f"An error occured while processing {folder}. Continuing...")
    if errors:
        logger.error(f"\n{len(errors)} out of {len(folders)} folders terminated with errors.")
        for folder, exc in errors:
            logger.error(f"\nIn {folder}", exc_info=exc)


def find_subfolders(path, name):
    """Breadth-first search for sub-folders called `name`, not descending into matches."""
    found, queue, seen = [], deque([Path(path)]), set()
    while queue:
        cur = queue.popleft()
        if cur.is_dir() and cur not in seen:
            seen.add(cur)
            if cur.name == name:
                found.append(str(cur))
            else:
                queue.extend(cur.iterdir())
    return found


def run_recursive(args):
    sub = find_subfolders(args.input_folder, "images")
    logger.info(f"Found {len(sub)} subfolder(s):\n-" + "\n-".join(sub))
    args.recursive = False
    run_in_folders(args, sub)


def run_from_file(args):
    try:
        with open(args.input_folder, "r") as f:
            folders = [line.strip() for line in f]
    except FileNotFoundError:
        logger.error(f"Unable to find the file {args.input_folder}")
        return 1
    except IsADirectoryError:
        logger.error(f"{args.input_folder} is a directory, please provide a file instead.")
        return 1
    folders = [Path(f) for f in dict.fromkeys(folders) if f.strip()]
    bad = [f for f in folders if not f.is_dir()]
    for f in bad:
        logger.error(f"[Error] Not a directory or does not exist: {f}")
    if bad:
        return 1
    args.from_file = False
    run_in_folders(args, folders)


def main(argv=None):
    """Entry point.  Multi-GPU: `python -m torch.distributed.run --nproc-per-node N -m deepfly3d_amd.cli INPUT ...`
    (one process per GPU; frames are sharded, rank 0 writes the result)."""
    import os

    args = parse_cli_args(argv)
    setup_logger(args)
    if args.debug:
        return print_debug(args)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist

        from . import distributed as dd

        _, _, local_rank = dd.init_from_env()
        args.device = str(dd.local_device(local_rank))
        try:
            return _dispatch(args)
        finally:
            dist.barrier()
            dist.destroy_process_group()
    return _dispatch(args)


def _dispatch(args):
    if args.from_file and args.recursive:
        logger.error('Error: choose an input method between "from file" and "recursive" but not both.')
        return 1
    if args.recursive:
        return run_recursive(args)
    if args.from_file:
        return run_from_file(args)
    return run(args)


if __name__ == "__main__":
    sys.exit(main())
