"""Constants of the fly set-up (values from reference df3d/config.py:15-69 and df3d/skeleton_fly.py)."""
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

config = {
    "name": "fly",
    "num_cameras": 7,                 # reference config.py:17
    "heatmap_shape": [64, 128],       # reference config.py:18
    "left_cameras": [0, 1, 2],
    "right_cameras": [6, 5, 4],
    "num_stacks": 2,                  # reference config.py:33
    "flip_cameras": [4, 5, 6],
    "num_joints": 38,                 # reference skeleton_fly.py (2 x 19)
    "num_predict": 19,                # reference config.py:36
    "input_shape": [256, 512],        # network input (rows, cols): 4 x the heat-map
    "calib_path": os.path.join(_HERE, "data", "calib.npz"),                       # reference data/calib.pkl
    "procrustes_template": os.path.join(_HERE, "data", "procrustes_template.npz"),  # reference data/df3d_result.pkl
    "procrustes_apply": True,
    # frames per bundle-adjustment problem on the Core/CLI path (0 = no limit): longer recordings are sub-sampled
    # with an even stride (camera_network.py:bundle_adjust)
    "ba_max_images": 1000,
}

# tracked-point class per joint of ONE side (19 joints): 3 legs x (body-coxa, coxa-femur, femur-tibia,
# tibia-tarsus, tarsus-tip), antenna, 3 stripes           (reference skeleton_fly.py:16-55)
BODY_COXA, COXA_FEMUR, FEMUR_TIBIA, TIBIA_TARSUS, TARSUS_TIP, ANTENNA, STRIPE = range(7)
TRACKED_SIDE = [BODY_COXA, COXA_FEMUR, FEMUR_TIBIA, TIBIA_TARSUS, TARSUS_TIP] * 3 + [ANTENNA, STRIPE, STRIPE, STRIPE]
TRACKED = TRACKED_SIDE * 2


# ---- pictorial-structures correction.  The bone prior is the reference's `bone_param`
# (df3d/skeleton_fly.py:252-261): length mean 0.9, deviation 0.3 for every joint that ends a leg segment, "no bone" for
# body-coxa, antenna and stripe joints.
BONE_MEAN, BONE_STD = 0.9, 0.3
PICTORIAL_DEFAULTS = {
    "num_peaks": 10,        # K: the reference's `num_peak` (at most 16)
    "num_proposals": 64,    # M: proposals kept per (frame, joint) (at most 256)
    "tau": 30.0,            # pixels: the number the reference carries as `alpha_reproj`
    "w_reproj": 1.0,
    "w_heatmap": 1.0,
    "w_bone": 1.0,
}

# ---- tracking of the 2-D detections through time: per (camera, network joint), the sequence of heat-map peaks
# that is jointly best over the recording.  tau truncates the squared jump between consecutive frames (pixels; the number section 9
# truncates its reprojection term at), w_motion weighs that jump and w_value the heat-map value a peak gives up against the frame's
# best; block_frames is the time block of the solve and changes no bit of the result.  tau and the two weights are guesses: nobody has
# measured them on a recording.
TRACK_DEFAULTS = {
    "tau": 30.0,
    "w_motion": 1.0,
    "w_value": 1.0,
    "block_frames": 256,
}
TRACK_WEIGHT_MAX = 1024.0
TRACK_BLOCK_FRAMES_RANGE = (1, 4096)
TRACK_NUM_PEAKS_RANGE = (1, 16)

# ---- suspect detections: joint j of a frame is flagged when its largest per-camera reprojection error
# exceeds REPROJ_THR[j] pixels.  The reference's `config["reproj_thr"]` (df3d/config.py:41): 40 for each of the 38 joints.
REPROJ_THR = np.full(38, 40.0, dtype=np.float64)

# ---- consensus triangulation: a subset of a joint's views qualifies when every one of its cameras reprojects
# the subset's own DLT point within ROBUST_TAU[j] pixels, and it must hold at least ROBUST_MIN_VIEWS cameras (2 .. 8).  20 px for each
# of the 38 joints is a guess: nobody has measured it on a recording.
ROBUST_TAU = np.full(38, 20.0, dtype=np.float64)
ROBUST_MIN_VIEWS = 2
ROBUST_MIN_VIEWS_RANGE = (2, 8)

# ---- robust-loss bundle adjustment: calibrate_calc's loss on the reprojection residuals, with scipy's meaning of
# least_squares(loss=, f_scale=).  'linear' is the reference's plain sum of squares; of the others 'soft_l1' is the one to use (huber and
# cauchy can stall at a perturbed start).  BA_F_SCALE, pixels, is where a residual stops counting in full: 4 px is about two standard
# deviations of the quantisation of a 7.5 px heat-map cell (7.5 / sqrt(12)) -- a guess that nobody has measured on a recording.  It is
# used only when a robust loss is asked for.
BA_LOSSES = ("linear", "soft_l1", "huber", "cauchy", "arctan")
BA_LOSS = "linear"
BA_F_SCALE = 4.0

# ---- trajectory triangulation: per joint, the 3-D points of a whole recording minimise the Huber loss
# (TRAJECTORY_HUBER pixels) of every view's reprojection error plus TRAJECTORY_LAMBDA[j] (px^2 / mm^2) times the squared second
# differences of the trajectory.  The two defaults come from a sweep of tests/trajectory_oracle.py on planted trajectories (section 24
# holds it) and are guesses: nobody has measured them on a recording.  Segments bridge at most REPAIR_MAX_GAP frames without a pair
# of views unless max_gap says otherwise.  The damped Gauss-Newton iteration starts at TRAJECTORY_MU_INIT, divides the damping by 10
# after an accepted trial (never below TRAJECTORY_MU_MIN: a frame no camera sees needs it when lambda is 0) and multiplies it by 10
# after a rejected one; a trial is accepted when its cost is at most (1 + TRAJECTORY_SLACK) times the cost before; a chain has
# converged when no coordinate of a step moves by TRAJECTORY_STEP_TOL mm, has stalled when the damping passes TRAJECTORY_MU_MAX and is
# out of iterations after TRAJECTORY_MAX_ITER trials.  trajectory_block_frames(T) frames are one lane's share of the banded solve: the
# lanes' interiors are serial in the block's frames and the separators' system in the number of blocks, so the block grows with the
# square root of the recording (32 frames at 1 000, the best of DESIGN.md section 24's table) and both serial parts with it.
TRAJECTORY_LAMBDA = np.full(38, 1e3, dtype=np.float64)
TRAJECTORY_HUBER = 10.0
TRAJECTORY_MU_INIT = 1e-3
TRAJECTORY_MU_MIN = 1e-6
TRAJECTORY_MU_MAX = 1e12
TRAJECTORY_SLACK = 1e-12
TRAJECTORY_STEP_TOL = 1e-8
TRAJECTORY_MAX_ITER = 300
TRAJECTORY_BLOCK_FRAMES_RANGE = (3, 1 << 20)
TRAJECTORY_MAX_FRAMES = 1 << 20


def trajectory_block_frames(frames):
    """The default block of the trajectory fit's banded solve for a recording of `frames` frames: ceil(sqrt(frames)), within the range."""
    lo, hi = TRAJECTORY_BLOCK_FRAMES_RANGE
    return int(min(max(lo, int(np.ceil(np.sqrt(max(int(frames), 0))))), hi))


# ---- heat-map triangulation: the 3-D point of a joint is where the product of its views' heat-maps, sampled at
# the point's projection, is largest.  The search starts at the plain triangulation and scores HEATMAP3D_GRID^3 points of a cube of
# half width HEATMAP3D_HALF (mm) around it, then of the cube around the best point with the step as its half width, HEATMAP3D_LEVELS
# times: the last step is 2 half / 8 / 4^(levels - 1), 0.0016 mm at the defaults.  A heat-map cell at or below HEATMAP3D_FLOOR (or not
# finite) counts as the floor: a view says "no information" there, it does not veto.  The three defaults come from planted blobs on
# the golden calibration (section 25 holds the table) and are guesses: nobody has measured them on a recording.
HEATMAP3D_GRID = 8          # a compile-time constant of csrc/heatmap3d.hip
HEATMAP3D_HALF = 0.4
HEATMAP3D_LEVELS = 4
HEATMAP3D_LEVELS_RANGE = (1, 6)
HEATMAP3D_FLOOR = 1e-3

# ---- per-camera frame lags from epipolar consistency: for every pair of cameras that share a joint, camera a's
# frame t is paired with camera b's frame t + d for every lag |d| <= SYNC_MAX_LAG; the squared Sampson distance of every such sample
# against the pair's fundamental matrix, truncated at SYNC_TAU^2 (pixels; the consensus stage's guess), is summed per window of
# SYNC_WINDOW frames, and the lag of a pair is the path through the windows that minimises those sums plus SYNC_SWITCH (px^2) per frame
# of lag changed between neighbouring windows.  A pair exists when both cameras detect some joint in at least SYNC_MIN_COUNT frames,
# and a window's margin is reported only where the chosen lag has that many samples.  SYNC_SWITCH and SYNC_MIN_COUNT were chosen on the
# planted recordings of tests/sync_cases.py (section 28 holds the margins); all five are guesses: nobody has measured them on a
# recording.
SYNC_MAX_LAG = 8
SYNC_MAX_LAG_RANGE = (0, 64)
SYNC_WINDOW = 256
SYNC_TAU = 20.0
SYNC_TAU_MAX = 4096.0
SYNC_SWITCH = 64.0
SYNC_SWITCH_MAX = float(1 << 24)
SYNC_MIN_COUNT = 16
SYNC_COST_SCALE = 1024   # an integer cost is the squared Sampson distance in units of 2^-10 px^2 (csrc/sync.hip: COST_SCALE)
SYNC_MAX_FRAMES = 1 << 20


# ---- leg joint angles.  Leg L = 3 side + l (l = 0, 1, 2: front, mid, hind) owns the five joints
# 19 side + 5 l + k; its eight angles come in this order: thorax-coxa yaw, pitch and roll, coxa-trochanter pitch and roll,
# femur-tibia pitch and roll, tibia-tarsus pitch; its four segment lengths are coxa, femur, tibia, tarsus.
LEG_NAMES = ["side0_front", "side0_mid", "side0_hind", "side1_front", "side1_mid", "side1_hind"]
LEG_ANGLE_NAMES = ["thc_yaw", "thc_pitch", "thc_roll", "ctr_pitch", "ctr_roll", "fti_pitch", "fti_roll", "tita_pitch"]


def leg_joints(leg):
    """The five joint ids (body-coxa, coxa-femur, femur-tibia, tibia-tarsus, tarsus tip) of leg `leg` (0..5)."""
    leg = int(leg)
    if not 0 <= leg < len(LEG_NAMES):
        raise ValueError(f"no leg {leg}")
    side, l = divmod(leg, 3)
    return [config["num_predict"] * side + 5 * l + k for k in range(5)]


# ---- constant-length legs: the most Newton iterations ops.fit_legs / --rigid-legs give a leg.  The golden
# recording needs 5 at the most; a leg that is still moving after 30 reports status 1.
RIGID_LEGS_MAX_ITER = 30


# ---- Morlet wavelet spectrograms of the joint angles.  The default bank: SPECTROGRAM_NUM_FREQS frequencies
# spaced geometrically from SPECTROGRAM_F_MIN Hz to fps * SPECTROGRAM_F_MAX_OVER_FPS (a quarter of the sampling rate: above it the
# negative-frequency image of a real series folds into the row), a wavelet of SPECTROGRAM_OMEGA0 radians per deviation cut at
# SPECTROGRAM_RADIUS deviations.  SPECTROGRAM_FPS stands in where the recording's frame rate is unknown (Core.get_fps() is None).
# SPECTROGRAM_TILE is the number of consecutive times one block of the kernel owns, SPECTROGRAM_MAX_SUPPORT the cap on K_i.
SPECTROGRAM_F_MIN = 1.0
SPECTROGRAM_F_MAX_OVER_FPS = 0.25
SPECTROGRAM_NUM_FREQS = 25
SPECTROGRAM_OMEGA0 = 5.0
SPECTROGRAM_RADIUS = 6.0
SPECTROGRAM_FPS = 100.0
SPECTROGRAM_TILE = 320
SPECTROGRAM_MAX_SUPPORT = 2048
# the angles of LEG_ANGLE_NAMES that live on the full circle and are unwrapped along time before the transform
SPECTROGRAM_UNWRAPPED_ANGLES = ("thc_pitch", "thc_roll", "ctr_roll", "fti_roll")


# ---- t-SNE behaviour maps of the angle spectrograms.  Every frame's spectrum is normalised to a distribution
# with BEHAVIOUR_FLOOR added to every channel (a silent channel must not make a divergence infinite); at most BEHAVIOUR_MAX_POINTS
# frames, spread evenly over the valid ones, are embedded by BEHAVIOUR_ITERATIONS steps of descent (the first
# BEHAVIOUR_EXAGGERATION_ITERATIONS of them with P multiplied by 12) and the others are placed among them.  BEHAVIOUR_POINTS_CAP
# is the most max_points may ask for: the dense N x N float64 tables are 2 GB each there.  BEHAVIOUR_PERPLEXITY is the effective
# number of neighbours of a frame; its entropy is met to BEHAVIOUR_ENTROPY_TOL nats by a beta in (0, BEHAVIOUR_BETA_MAX].
BEHAVIOUR_FLOOR = 1e-9
BEHAVIOUR_MAX_POINTS = 8192
BEHAVIOUR_POINTS_CAP = 16384
BEHAVIOUR_PERPLEXITY = 32.0
BEHAVIOUR_ENTROPY_TOL = 1e-10
BEHAVIOUR_BETA_MAX = 1e12
BEHAVIOUR_ITERATIONS = 1000
BEHAVIOUR_EXAGGERATION_ITERATIONS = 250

# ---- segmentation of the behaviour map.  The density of the map is a sum of Gaussians of deviation
# BEHAVIOUR_DENSITY_SIGMA_FRACTION times the map's larger extent, on a square grid of BEHAVIOUR_GRID x BEHAVIOUR_GRID cells that
# reaches three deviations past the outermost frames; a peak of the density founds a region when it reaches BEHAVIOUR_MIN_PEAK of
# the highest.
BEHAVIOUR_GRID = 256
BEHAVIOUR_GRID_RANGE = (2, 1024)
BEHAVIOUR_DENSITY_SIGMA_FRACTION = 1.0 / 32.0
BEHAVIOUR_MIN_PEAK = 0.01

# ---- gait analysis of the leg tips.  A tip's velocity is the central difference over GAIT_DIFF_HALF frames
# to either side (clipped at the recording's ends; within GAIT_DIFF_HALF_RANGE).  A leg goes into swing when its anterior velocity
# rises above GAIT_SWING_ON and into stance when it falls below GAIT_SWING_OFF, in pose units (mm) per second; in between it keeps
# its state.  The two defaults are a guess from published tip speeds of walking flies: nobody has measured them on a real recording.
# GAIT_TRIPODS: the swing masks (bit L = leg L) of the two tripods, legs 0, 2, 4 and legs 1, 3, 5.
GAIT_DIFF_HALF = 2
GAIT_DIFF_HALF_RANGE = (1, 64)
GAIT_SWING_ON = 5.0
GAIT_SWING_OFF = 0.0
GAIT_TRIPODS = (21, 42)

# ---- repair of the 3-D pose.  A joint is an outlier when, in any coordinate, it lies further from the median
# of the REPAIR_HALF_WINDOW frames to either side (clipped at the recording's ends, missing frames left out) than REPAIR_THRESHOLD
# times 1.4826 times the median absolute deviation of that window, and further than REPAIR_FLOOR pose units (mm); a window with
# fewer than REPAIR_MIN_COUNT frames is not tested.  Missing joints and outliers are then interpolated linearly between their nearest
# good neighbours where the gap is at most REPAIR_MAX_GAP frames long, and left (removed) otherwise.  The four defaults are guesses
# in the sense of the gait thresholds: nobody has measured them on a real recording.  A test on positions is blind to a spike smaller
# than the threshold times the local spread of a fast-moving tip.
REPAIR_HALF_WINDOW = 5
REPAIR_HALF_WINDOW_RANGE = (1, 64)
REPAIR_THRESHOLD = 6.0
REPAIR_FLOOR = 0.05
REPAIR_MIN_COUNT = 3
REPAIR_MAX_GAP = 10
REPAIR_MAX_GAP_RANGE = (0, 1000000)
REPAIR_MAD_TO_SIGMA = 1.4826   # the median absolute deviation of a normal sample times this estimates its standard deviation

# ---- the treadmill ball and the fictive path.  One sphere is fitted to the stance tips of a recording; with a
# known radius its centre takes BALL_FIT_ITERATIONS Gauss-Newton steps (within BALL_FIT_ITERATIONS_RANGE) from the algebraic centre.
# A fit is refused where a Cholesky pivot of its normal matrix is at or below BALL_PIVOT_MIN times the largest diagonal entry; a
# frame's rotation is NaN with fewer than BALL_MIN_LEGS stance legs (within BALL_MIN_LEGS_RANGE; one leg leaves the spin about its own
# radius free) or with a pivot at or below BALL_FRAME_PIVOT_MIN times the trace.  Each default is a guess: the 8 steps were enough on
# planted data alone (the step fell below 1e-12 by step 7 at 0.1 mm of tip noise), and nobody has measured any of them on a recording.
BALL_FIT_ITERATIONS = 8
BALL_FIT_ITERATIONS_RANGE = (1, 64)
BALL_PIVOT_MIN = 1e-10
BALL_MIN_LEGS = 2
BALL_MIN_LEGS_RANGE = (2, 6)
BALL_FRAME_PIVOT_MIN = 1e-10

# ---- which camera sees which joint (reference df3d/skeleton_fly.py:202-250), by camera id: cameras 0-2 look at the side whose
# joints are 0..18, cameras 4-6 at the side of joints 19..37, camera 3 faces the fly.  Pinned by tests/golden/skeleton_tables.npz.
# Where df3d::relayout_source (csrc/geometry_dev.h) fills a joint of a side camera under the identity ordering, this table sees it;
# the table also lists the antenna for cameras 2 and 4, which the re-layout leaves at zero (as the reference's own does).
FRONT_CAMERA = 3
IGNORE_JOINT_ID = [j for j, kind in enumerate(TRACKED) if kind in (BODY_COXA, COXA_FEMUR, ANTENNA)]   # the reference's ignore_joint_id


def camera_see_joint(cam_id, joint_id):
    """Whether camera `cam_id` (0..6; 7 is an alias of the front camera, as in the reference) can see joint `joint_id` (0..37)."""
    cam_id = FRONT_CAMERA if cam_id == 7 else int(cam_id)
    if not 0 <= cam_id < config["num_cameras"]:
        raise NotImplementedError(f"no camera {cam_id}")
    kind, limb = TRACKED[joint_id], limb_of_joint(joint_id)
    if cam_id == FRONT_CAMERA:   # the front two legs of both sides from the femur-tibia joint on, and the antennae
        return limb % 5 in (0, 1, 3) and kind not in (BODY_COXA, COXA_FEMUR)
    if (limb >= 5) != (cam_id > FRONT_CAMERA):   # a side camera sees its own side only
        return False
    return not (cam_id in (2, 4) and kind == STRIPE)   # the two rear cameras cannot see the stripes


def bone_tree():
    """(parent [38] int32, bone [38, 2] float64 (mean, deviation)) from TRACKED: a coxa-femur, femur-tibia, tibia-tarsus or
    tarsus-tip joint hangs from the joint before it; every other joint is a root.  6 chains of 5 joints + 8 single joints."""
    parent = np.full(len(TRACKED), -1, dtype=np.int32)
    bone = np.zeros((len(TRACKED), 2), dtype=np.float64)
    for j, kind in enumerate(TRACKED):
        if kind in (COXA_FEMUR, FEMUR_TIBIA, TIBIA_TARSUS, TARSUS_TIP):
            parent[j] = j - 1
            bone[j] = (BONE_MEAN, BONE_STD)
    return parent, bone


def load_calibration():
    """{cam_id: {R, tvec, intr, distort}} as in the reference's data/calib.pkl."""
    d = np.load(config["calib_path"])
    return {c: {"R": d["R"][c].copy(), "tvec": d["tvec"][c].copy(), "intr": d["intr"][c].copy(), "distort": d["distort"][c].copy()} for c in range(7)}


def load_procrustes_template():
    return np.load(config["procrustes_template"])["points3d"]


# ---- drawing tables of the 38-joint skeleton (what pyba.config.df3d_bones / df3d_colors hold for the reference's
# Core.plot_2d, reference df3d/core.py:311-319).  Joints of one side: three legs of five joints, antenna, three stripes.
def skeleton_bones():
    """[[joint_a, joint_b], ...]: consecutive joints of every leg and of the stripe chain, both sides."""
    bones = []
    for side in (0, 19):
        for leg in range(3):
            bones += [[side + 5 * leg + k, side + 5 * leg + k + 1] for k in range(4)]
        bones += [[side + 16, side + 17], [side + 17, side + 18]]
    return bones


def limb_of_joint(joint):
    """Limb id 0..9: right-side view legs 0-2, antenna 3, stripes 4; the other side 5-9."""
    side, j = divmod(joint, 19)
    return 5 * side + (j // 5 if j < 15 else 3 if j == 15 else 4)


_REDS = [(186, 30, 49), (201, 86, 79), (213, 133, 121)]
_BLUES = [(15, 115, 153), (26, 141, 175), (117, 190, 203)]
_GREY = (210, 210, 210)
LIMB_COLORS = _REDS + [_GREY, _GREY] + _BLUES + [_GREY, _GREY]


# ---- heat-map overlays: which of a camera's 19 heat-map planes is which joint of the 38-joint layout.  The
# rule is the re-layout's (reference df3d/core.py:187-203; df3d::relayout_source in csrc/geometry_dev.h), keyed like it on the
# camera's POSITION in the camera ordering: positions 0-2 fill joints 0..18, positions 4-6 joints 19..37 and are the views the network
# sees mirrored, positions 2 and 4 leave antenna and stripes out, position 3 (the front camera) fills nothing.
def camera_position(cam_id, camera_ordering=None):
    """Position of camera `cam_id` in `camera_ordering` (default: the identity ordering, where it is the camera id)."""
    order = list(range(config["num_cameras"])) if camera_ordering is None else [int(c) for c in camera_ordering]
    if int(cam_id) not in order:
        raise NotImplementedError(f"no camera {cam_id}")
    return order.index(int(cam_id))


def camera_is_flipped(cam_id, camera_ordering=None):
    """Whether the network sees camera `cam_id` mirrored (Core.pose2d_estimation's flip set: the cameras after position 3)."""
    return camera_position(cam_id, camera_ordering) > 3


def heatmap_planes(cam_id, joints=(), camera_ordering=None):
    """[(plane, joint), ...]: the heat-map planes (0..18) of camera `cam_id` and the joint of the 38-joint layout each of them becomes
    under the re-layout, in plane order.  `joints` (plot_2d's ids) keeps only the listed joints; a joint the camera does not fill is
    dropped, and the front camera has no planes.  A plane's colour is plane_color(joint)."""
    pos = camera_position(cam_id, camera_ordering)
    keep = None if not len(joints) else {int(j) for j in joints}
    pairs = []
    for plane in range(config["num_predict"]):
        if pos == 3 or (pos in (2, 4) and plane >= 15):
            continue
        joint = plane if pos < 3 else plane + config["num_predict"]
        if keep is None or joint in keep:
            pairs.append((plane, joint))
    return pairs


def plane_color(joint):
    """RGB of the heat-map plane of joint `joint`: its limb's colour, as plot_2d and the pose videos draw the joint."""
    return LIMB_COLORS[limb_of_joint(joint) % len(LIMB_COLORS)]
