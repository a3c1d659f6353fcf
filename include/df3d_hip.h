/*
 * df3d_hip.h -- C ABI of libdf3d_hip.so, the MI355X (gfx950) back-end of the DeepFly3D per-frame hot
 * path.  Plain C: pointers, sizes, no torch / C++ types.  This is the drop-in boundary: every entry
 * point replaces one piece of work the reference reaches through its two Python imports
 *     from df2d.inference import inference_folder        (reference df3d/core.py:11)
 *     from pyba.CameraNetwork import CameraNetwork       (reference df3d/core.py:12)
 * The reference has no FFI of its own; INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every pointer named *_dev is DEVICE memory owned by the caller (a torch tensor's data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are asynchronous
 *     on that stream unless the comment says "synchronous".
 *   - return value: 0 = DF3D_OK, negative = error; df3d_last_error() returns a thread-local message.
 *   - no exceptions cross the ABI; handles are not thread-safe, distinct handles are independent.
 */
#ifndef DF3D_HIP_H
#define DF3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DF3D_OK 0
#define DF3D_EINVAL (-1)  /* bad argument                       */
#define DF3D_EHIP (-2)    /* a HIP runtime call failed          */
#define DF3D_ESTATE (-3)  /* handle not ready (weights missing) */
#define DF3D_ENOGPU (-4)  /* no gfx950 device visible           */
#define DF3D_ENOSPC (-5)  /* the caller's buffer is too small (the size needed was reported) */
#define DF3D_EIO (-6)     /* a file could not be opened or read */

#define DF3D_DTYPE_F32 0
#define DF3D_DTYPE_BF16 1
#define DF3D_DTYPE_F16 2  /* IEEE half activations + weights, fp32 accumulate: the bf16 engine's kernels on the other 16-bit format */
#define DF3D_DTYPE_F32S 3 /* float32 tensors, weights and accumulation -- the F32 engine's plan, workspace and kernels -- with every product formed on the
                             half-precision matrix pipe from a two-way IEEE-half split of both operands (x = hi + lo to 2^-22 |x|): three MFMAs per
                             K step (hi hi + lo hi + hi lo, the 2^-22 lo lo term dropped) where exact fp32 takes eight four times as long.  Operands
                             must lie inside the half range (|x| < 65 504), which batch-normalised activations and their weights do.  Not
                             bit-identical to F32: heat-maps differ by ~1.5e-6 of their range (the same 5e-5 test tolerance, the same arg-max cells).
                             Needs the df3d_hg_lowp_bytes() buffer (the pre-split copy of the weights and the streams packed from it) */

const char* df3d_last_error(void);
/* ABI revision of the library: DF3D_ABI_VERSION of the header it was built from.  It changes whenever an entry point's signature or
 * a struct layout does (round 3 inserted `resize` into df3d_preprocess_u8 / df3d_hg_forward_u8 and `bytes_m1` into
 * df3d_hg_profile_read: 300; round 4: 400; round 5 added df3d_ba_lsmr_form and grew df3d_ba_lsmr_work_doubles: 500; round 6 added df3d_hg_profile_executed_flops and df3d_heatmap_argmax_checked: 600, and the df3d_ba_trf_* entries: 610); a caller compares it with the header it compiled against before its first call
 * (deepfly3d_amd/_native.py:load does). */
#define DF3D_ABI_VERSION 610
int df3d_version(void);
/* number of visible HIP devices (<0 on error); name of device `dev` copied to buf */
int df3d_device_count(void);
int df3d_device_name(int dev, char* buf, int buflen);

/* ------------------------------------------------------------------------------------------------
 * a1  input front-end of df2d's inference_folder (call site reference df3d/core.py:177-185): uint8 frames
 *     [n, H, W, C] (C = 1 or 3) -> float32 NHWC [n, OH, OW, 3]: optional left-right flip per view
 *     (flip_dev[n] uint8, may be NULL; the reference flips cameras ordering[4:]), resize, (v/255 - mean[c]) / std[c].
 *     mean3/std3 are HOST float[3].  df2d's resize rule is not in the reference checkout, so it is an argument:
 *     DF3D_RESIZE_BILINEAR (half-pixel centres, no antialias: cv2.INTER_LINEAR), DF3D_RESIZE_BILINEAR_ALIGN_CORNERS,
 *     DF3D_RESIZE_AREA (overlap-weighted mean of the covered source rectangle: cv2.INTER_AREA).
 *     (Round 3 added the `resize` argument to this function and to df3d_hg_forward_u8.)
 * ---------------------------------------------------------------------------------------------- */
#define DF3D_RESIZE_BILINEAR 0
#define DF3D_RESIZE_BILINEAR_ALIGN_CORNERS 1
#define DF3D_RESIZE_AREA 2
int df3d_preprocess_u8(const unsigned char* img_dev, const unsigned char* flip_dev, int n, int H, int W, int C,
                       float* out_dev, int OH, int OW, const float* mean3_host, const float* std3_host, int resize, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a1  JPEG front-end: n baseline JPEG files -> their luma planes, on the device.
 *     Replaces the libjpeg decode inside df2d's DataLoader (call site reference df3d/core.py:177-185; the
 *     frames are ffmpeg-written JPEGs, df3d/core.py:446-459).  Baseline / extended sequential Huffman, 8 bit,
 *     1-4 components in one interleaved scan, any sampling factors, restart intervals; libjpeg's default
 *     "islow" inverse DCT, bit-exact.  Only the first (luma) component is reconstructed.
 * files_dev   the files' bytes in one 16-byte aligned buffer of total_file_bytes (+ 16 readable bytes behind it);
 *             file i = [offsets[i], offsets[i] + sizes[i]), every offset a multiple of 16, files in
 *             ascending, non-overlapping order
 * offsets_dev, sizes_dev  [n] uint32 (device);  max_file_bytes = the largest size (host value, 0 = unknown; a hint kept
 *             for callers of round 1, whose parallel decoder staged small streams in LDS: the decoder now keeps each lane's
 *             next stream dwords in registers and ignores it)
 * luma_dev    [n, height, width] uint8;   every file must be width x height
 * status_dev  [n] int32: 0 ok, 1 truncated, 2 not a JPEG, 3 unsupported (progressive / arithmetic / 12 bit /
 *             multi-scan), 4 corrupt, 5 size differs.  Planes of failed files are left untouched.
 * path_dev    optional [n] int32 (may be NULL): > 0 = decoded by the parallel Huffman kernel (the value is its number of
 *             synchronisation passes); <= 0 = by the sequential one (0: restart intervals / sequential requested / table
 *             problem, -1: no convergence, -2: stream ends early, -3: invalid symbols)
 * work_dev    >= df3d_jpeg_work_bytes(n, width, height, total_file_bytes) bytes, 256-byte aligned
 * flags       0, or DF3D_JPEG_SEQUENTIAL: skip the parallel (self-synchronising) Huffman kernel and decode every
 *             file with the sequential wave-per-file kernel (the exact fall-back the parallel one defers to for
 *             restart-interval, truncated or invalid streams); results are identical either way
 * ---------------------------------------------------------------------------------------------- */
#define DF3D_JPEG_SEQUENTIAL 1
size_t df3d_jpeg_work_bytes(int n, int width, int height, size_t total_file_bytes);
int df3d_jpeg_decode_luma(const unsigned char* files_dev, const unsigned* offsets_dev, const unsigned* sizes_dev, int n,
                          size_t total_file_bytes, unsigned max_file_bytes, int width, int height, unsigned char* luma_dev, int* status_dev,
                          int* path_dev, void* work_dev, size_t work_bytes, int flags, void* stream);

/* Host helper of the JPEG front-end (no device work): read n files with `threads` native threads into one staging buffer
 * (pinned host memory, typically) in the layout df3d_jpeg_decode_luma takes: file i at starts[i] (a multiple of 16, path
 * order, padding zeroed), sizes[i] bytes; *total_bytes = the bytes the layout needs (16 readable bytes follow it).  Returns
 * DF3D_ENOSPC, with *total_bytes set and nothing read, when dst is NULL or dst_bytes < *total_bytes + 16; DF3D_EIO (and the
 * path in df3d_last_error()) when a file cannot be opened or read.  The reference reads its frames one per DataLoader
 * worker call (df2d, behind reference df3d/core.py:177-185). */
int df3d_read_files(const char* const* paths, int n, unsigned char* dst, size_t dst_bytes, unsigned* starts, unsigned* sizes,
                    size_t* total_bytes, int threads);

/* ------------------------------------------------------------------------------------------------
 * a1' JPEG encoder: n RGB frames -> the entropy-coded scans of their baseline JPEG files, on
 *     the device; libjpeg's arithmetic (integer colour conversion, 4:2:0 with the h2v2 downsampler, the "islow"
 *     forward DCT, the Annex K Huffman tables, no restart markers), byte-equal to libjpeg's scan.  The header
 *     (SOI .. SOS) and EOI are the host's (deepfly3d_amd/jpeg.py: jfif_header).
 * rgb_dev     [n, h, w, 3] uint8, packed; w and h 1 .. 65535.  Rows are read as dwords where 3 w is a multiple of 4
 *             and rgb_dev is 4-byte aligned, as bytes otherwise
 * qtab_luma, qtab_chroma   [64] host, natural order, every entry 1 .. 255
 * out_dev     [n, out_capacity_per_frame] uint8: frame i's scan starts at i * out_capacity_per_frame
 * sizes_dev   [n] int64: frame i's true scan size, also where it exceeds the capacity
 * status_dev  [n] int32: 0 ok, 1 the scan did not fit (nothing is written past the frame's slot; encode again with
 *             sizes_dev[i] bytes of room)
 * work_dev    >= df3d_jpeg_encode_work_bytes(n, w, h) bytes, 256-byte aligned (0 is returned for arguments the
 *             encoder refuses)
 * coef_out_dev  optional [n, blocks, 64] int16, 4-byte aligned (may be NULL): the quantised coefficients in zigzag
 *             order, blocks in scan order (per MCU: Y00 Y01 Y10 Y11 Cb Cr; blocks = 6 ceil(w/16) ceil(h/16)), dummy
 *             blocks filled by libjpeg's rule
 * bits_out_dev  optional [n, blocks] int32 (may be NULL): entropy-coded bits per block
 * ---------------------------------------------------------------------------------------------- */
size_t df3d_jpeg_encode_work_bytes(int n, int w, int h);
int df3d_jpeg_encode_rgb(const unsigned char* rgb_dev, int n, int h, int w, const unsigned char* qtab_luma, const unsigned char* qtab_chroma,
                         unsigned char* out_dev, size_t out_capacity_per_frame, long long* sizes_dev, int* status_dev, void* work_dev, size_t work_bytes,
                         short* coef_out_dev, int* bits_out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a3  heat-map -> point + confidence.   Replaces df2d's heatmap2points / confidence extraction behind
 *     inference_folder(..., return_confidence=True)          (reference df3d/core.py:177-185,
 *     semantics reference README.md:404: arg-max over (h, w), confidence = the max value).
 * hm_dev   [n, joints, h, w] float32 planes (NCHW, the reference's heat-map layout)
 * pts_dev  [n, joints, 2]    float32   (row / h, col / w)   -- the reference's normalised (row, col)
 * conf_dev [n, joints]       float32   the peak value
 * Ties resolve to the first index in row-major order.  h*w must be a multiple of 4.
 * ---------------------------------------------------------------------------------------------- */
int df3d_heatmap_argmax(const float* hm_dev, int n, int joints, int h, int w, float* pts_dev, float* conf_dev,
                        void* stream);
/* (round 6) the same, plus the overflow guard of the reduced-precision engines: *nonfinite_planes_dev (device int, zeroed by the caller, may be
 * NULL) is incremented once for every plane that holds an infinity or a NaN anywhere -- the kernel reads every value anyway.  The F16 and F32S
 * hourglass engines need every activation inside the IEEE-half range (|x| < 65 504); a trained checkpoint that leaves it turns into inf / NaN
 * heat-maps and, without this flag, into a silently wrong points2d / heatmap_confidence (the bar it protects: reference tests/test_df3d.py:167-178).
 * The host reads the counter once per recording (deepfly3d_amd/inference.py) and refuses the result, naming the dtype to rerun with. */
int df3d_heatmap_argmax_checked(const float* hm_dev, int n, int joints, int h, int w, float* pts_dev, float* conf_dev,
                                int* nonfinite_planes_dev, void* stream);
/* opt-in sub-pixel localisation (this project's own rule, restated in float64 by tests/subpixel_oracle.py and met
 * bit for bit): df3d_heatmap_argmax_checked whose point is the winning cell moved by the maximum of the quadratic through its 3 x 3
 * neighbourhood, at most half a cell per axis, evaluated in float64 and rounded once to float32.  A cell on the border of the plane, or
 * with an infinity or a NaN among the nine values, keeps df3d_heatmap_argmax's point exactly.  The cell, conf_dev and the counter are
 * those of df3d_heatmap_argmax_checked.  h and w must be powers of two. */
int df3d_heatmap_argmax_subpixel(const float* hm_dev, int n, int joints, int h, int w, float* pts_dev, float* conf_dev,
                                 int* nonfinite_planes_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a4  19 -> 38 joint re-layout and un-flip.   Replaces reference df3d/core.py:187-203.
 * pts19_dev [7, T, 19, 2] float32 (network order), ordering[7] HOST ints (camera_ordering),
 * out_dev   [7, T, 38, 2] float64 normalised (row, col).
 * ---------------------------------------------------------------------------------------------- */
int df3d_relayout_19_to_38(const float* pts19_dev, const int* ordering_host, int T, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a6  multi-view DLT triangulation.   Replaces pyba CameraNetwork.triangulate()
 *     (call site reference df3d/core.py:355).
 * P          [ncam, 3, 4] float64   K[R|t], pixel units (device OR host pointer; 84 doubles travel as
 *            a kernel argument)
 * pts_px_dev [ncam, T, J, 2] float64 (row_px, col_px); a camera sees (t, j) iff both are != 0
 * X_dev      [T, J, 3] float64; 0 where fewer than 2 cameras see the joint.      ncam <= 8.
 * ---------------------------------------------------------------------------------------------- */
int df3d_triangulate(const double* P, const double* pts_px_dev, int ncam, int T, int J, double* X_dev,
                     void* stream);
/* same, taking NORMALISED (row, col) detections and multiplying by (row_scale, col_scale) = (H, W) in the kernel,
 * i.e. the reference's `points2d * image_shape[::-1]` (df3d/core.py:247) fused into the triangulation */
int df3d_triangulate_scaled(const double* P, const double* pts_norm_dev, double row_scale, double col_scale, int ncam,
                            int T, int J, double* X_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a6b pictorial-structures correction of the 2-D detections (the model is this project's own
 *     specification, restated in float64 by tests/pictorial_oracle.py).  All three run asynchronously on `stream` and validate
 *     their arguments before they touch the device.
 * df3d_heatmap_peaks: the k (1..16) best local maxima of every [h, w] plane (powers of two, 64 <= h*w <= 8192), value descending then
 *     flat index ascending.  A cell is a peak when its value is finite, > every finite 8-neighbour before it in row-major order and
 *     >= every finite one after it; peak 0 is then df3d_heatmap_argmax's cell whenever the plane's maximum is finite.
 *     count_dev [n, joints] int32 (<= k); pts_dev [n, joints, k, 2] float32 (row / h, col / w); val_dev [n, joints, k] float32;
 *     unused slots are zero.
 * df3d_ps_proposals: frames [t0, t0 + tn) of a T-frame recording.  P_host [7, 3, 4] HOST float64 (pixels, physical cameras),
 *     ordering_host[7] (camera_ordering), X0_dev [T, 38, 3] float64 = df3d_triangulate_scaled(P, argmax2d, img_h, img_w) of the
 *     re-layout of the arg-max detections (proposal 0: it IS df3d_triangulate's point), peak_*_dev [7, T, 19, ...]
 *     (df3d_heatmap_peaks of the network's planes), img_h / img_w the image size in pixels.  Per (frame, joint): proposal 0,
 *     proposal 1 + q k^2 + i k + j = the two-view DLT of peak i and peak j of the q-th pair of the cameras that see the joint;
 *     U = sum over those cameras of w_reproj min(d, tau)^2 / tau^2 - w_heatmap h (d, h: distance to and value of the nearest
 *     peak).  Kept: proposal 0, then the m - 1 (m <= 256) lowest U, ties to the lower index.  Outputs [tn, 38] kept_count,
 *     [tn, 38, m] kept_index (proposal index), kept_X [.., 3], kept_U, kept_match (byte a = the peak matched in the a-th seeing camera).
 * df3d_ps_solve: exact min-sum over the tree parent_host[38] (-1 = none; every joint parents at most one joint) with the bone
 *     cost w_bone ((|X_parent - X_j| - mu_j) / sigma_j)^2, bone_host [38, 2] = (mu, sigma), on df3d_ps_proposals' kept sets.
 *     Writes frames [t0, t0 + tn) of points2d_dev [7, T, 38, 2] (the matched peaks, un-flipped as the re-layout does; entries
 *     of cameras that do not see a joint copied from argmax2d), choice_dev [T, 38] (chosen proposal index) and energy_dev [T].
 *     work_dev: >= 38 * tn doubles.
 * ---------------------------------------------------------------------------------------------- */
int df3d_heatmap_peaks(const float* hm_dev, int n, int joints, int h, int w, int k, int* count_dev, float* pts_dev, float* val_dev,
                       void* stream);
/* df3d_heatmap_peaks with every peak's point refined by the rule of df3d_heatmap_argmax_subpixel (the neighbours come from the plane
 * in LDS): count, order and values are df3d_heatmap_peaks', and peak 0's point is df3d_heatmap_argmax_subpixel's bit for bit whenever
 * the plane's maximum is finite. */
int df3d_heatmap_peaks_subpixel(const float* hm_dev, int n, int joints, int h, int w, int k, int* count_dev, float* pts_dev,
                                float* val_dev, void* stream);
int df3d_ps_proposals(const double* P_host, const int* ordering_host, const double* X0_dev, const int* peak_count_dev,
                      const float* peak_pts_dev, const float* peak_val_dev, int T, int t0, int tn, int k, int m, double img_h,
                      double img_w, double tau, double w_reproj, double w_heatmap, int* kept_count_dev, int* kept_index_dev,
                      double* kept_X_dev, double* kept_U_dev, int* kept_match_dev, void* stream);
int df3d_ps_solve(const int* ordering_host, const int* parent_host, const double* bone_host, double w_bone, const double* argmax2d_dev,
                  const int* peak_count_dev, const float* peak_pts_dev, int T, int t0, int tn, int k, int m, const int* kept_count_dev,
                  const int* kept_index_dev, const double* kept_X_dev, const double* kept_U_dev, const int* kept_match_dev,
                  double* points2d_dev, int* choice_dev, double* energy_dev, double* work_dev, size_t work_doubles, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a6c per-joint reprojection errors and suspect-joint masks (the model is this project's own
 *     specification, restated in float64 by tests/reproj_oracle.py).  The first half of the reference's correction workflow
 *     (Core.next_error / joint_has_error, reference df3d/core.py:205-227, 481-507).
 * P_host [ncam, 3, 4] HOST float64 (pixels, no distortion: the DLT's model), pts_px_dev [ncam, T, J, 2] (row_px, col_px),
 *     X_dev [T, J, 3] (df3d_triangulate of the same detections on the Python paths; taken as given).  A camera is a view of
 *     (t, j) when both coordinates are non-zero.  With >= 2 views, every view c gets e = |P_c [X; 1] projected - (col, row)|
 *     in pixels (+inf when w <= 0 or the result is not finite); non-views, and every camera of a joint with < 2 views, get 0.
 * err_dev [ncam, T, J] (camera-major like points2d), jmax_dev [T, J] = max over cameras (may be NULL), mask_dev [T] int64:
 *     bit j set when jmax[t, j] > thr_host[j] (strict; thr_host [J] HOST float64, each >= 0 and not NaN, +inf disables j).
 * 1 <= ncam <= 8, 1 <= J <= 64, T >= 0 (T = 0: nothing to do).  Asynchronous on `stream`; arguments are validated before the
 *     device is touched.
 * ---------------------------------------------------------------------------------------------- */
int df3d_reproj_errors(const double* P_host, const double* pts_px_dev, const double* X_dev, int ncam, int T, int J,
                       const double* thr_host, double* err_dev, double* jmax_dev, long long* mask_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a6d temporal smoothing of the 2-D detections for display: reference df3d/signal_util.py:135-160
 *     `smooth_pose2d` (call site df3d/core.py:286-296), restated in float64 by tests/smooth_oracle.py.
 * pts_dev / out_dev [C, T, nch] float64 (nch = J * 2 contiguous doubles per frame); every (camera, channel) series is filtered
 *     along T on its own.  Output t looks at the `window` samples t - window/2 .. t + window/2 - 1 of the series extended by edge
 *     replication (frames before 0 read frame 0, frames after T - 1 read frame T - 1), takes their population standard deviation
 *     sqrt(mean((x - mean)^2)) and writes sum_k w_smooth[k] x[k] when it is below std_thr (strict), sum_k w_keep[k] x[k] otherwise
 *     (taps of w_keep that are exactly 0 are skipped).  A window that holds a NaN or an infinity has a NaN deviation and takes the
 *     keep taps.  w_smooth_host / w_keep_host [window] HOST float64, finite: a filter kernel folded onto the window (Python:
 *     ops.gaussian_window_taps; the reference's pair is sigma 7 and sigma 0.1, the latter the unit tap at window/2).
 * 1 <= C <= 8, 1 <= nch <= 128, window even in [2, 64], std_thr >= 0 and not NaN, T >= 0 (T = 0: nothing to do); out_dev must
 *     not overlap pts_dev.  One launch for all cameras, asynchronous on `stream`; arguments are validated before the device is
 *     touched.
 * ---------------------------------------------------------------------------------------------- */
int df3d_smooth_pose2d(const double* pts_dev, int C, long long T, int nch, int window, double std_thr, const double* w_smooth_host,
                       const double* w_keep_host, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a9  per-side Procrustes registration to the template pose + the `Core.get_points3d` chain.
 *     Replaces reference df3d/procrustes.py:51-151 (`procrustes_seperate`, call site df3d/core.py:358,340),
 *     df3d/plot_util.py:85-91 (`normalize_pose_3d`, call site core.py:341) and df3d/signal_util.py:69-100
 *     (`filter_batch`, call site core.py:342).  All float64, SEQUENCE-GLOBAL (medians over every frame): call
 *     once on the gathered sequence.  Several small launches on `stream`; `work` is caller-owned scratch.
 *
 * df3d_column_median : cols_dev [ncols] columns of n doubles, column c at cols_dev + c*col_stride;
 *                      out_dev[c] = median (exact order statistic; mean of the two middle values for even n).
 * df3d_procrustes    : pts_dev / out_dev [T, 38, 3]; tmpl_seg_med HOST [2][12] = per side, median over the
 *                      template's frames of the 12 leg-segment lengths; tmpl_fit_med HOST [2][6][3] = median of
 *                      the template's 6 fit joints (side joints 0,1,5,6,10,11).  work_dev >=
 *                      df3d_procrustes_work_doubles(T) doubles.
 * df3d_pose_normalize: out = in - median over all T*njoints points (per axis); rotate != 0 additionally maps
 *                      (x, y, z) -> (x, -z, -y).  work_dev >= 3 doubles; with >= 1024 doubles the medians of sequences of
 *                      more than 65 536 values per axis are taken by many workgroups (same values).  in == out allowed.
 * df3d_oneeuro_filter: in/out [T, nch]; one independent One-Euro filter per channel; sample i carries the time
 *                      stamp (i + first_stamp) * stamp_step and, like the reference, the filter re-derives its
 *                      sampling frequency from consecutive stamps.  The reference's `filter_batch` is
 *                      (freq 100, mincutoff 0.1, beta 2.0, dcutoff 1.0, first_stamp 1, stamp_step 0.1).
 *                      Bit-identical to the reference's float arithmetic.
 * ---------------------------------------------------------------------------------------------- */
int df3d_column_median(const double* cols_dev, int ncols, long long n, long long col_stride, double* out_dev, void* stream);
long long df3d_procrustes_work_doubles(long long T);
int df3d_procrustes(const double* pts_dev, long long T, const double* tmpl_seg_med, const double* tmpl_fit_med,
                    double* out_dev, double* work_dev, long long work_doubles, void* stream);
int df3d_pose_normalize(const double* in_dev, long long T, int njoints, int rotate, double* out_dev, double* work_dev,
                        long long work_doubles, void* stream);
int df3d_oneeuro_filter(const double* in_dev, long long T, int nch, double freq, double mincutoff, double beta,
                        double dcutoff, long long first_stamp, double stamp_step, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a10 leg joint angles and segment lengths from the 3-D pose (the model is this project's own
 *     specification, restated in float64 by tests/joint_angles_oracle.py).  The reference stops at the pose.
 * pts_dev [n, 38, 3] float64, the layout of points3d_wo_procrustes.  Leg L = 3 side + l owns joints 19 side + 5 l + k, k = 0..4
 *     (body-coxa .. tarsus tip).  A joint is missing when its three coordinates are exactly 0 or any of them is not finite.
 * df3d_body_frame: frame_dev [n, 3, 3], rows ex, ey, ez of each pose's own frame from its six body-coxa joints C[side][l]:
 *     ey along mean_l C[0][l] - mean_l C[1][l]; ex along the part perpendicular to ey of (C[0][0] + C[1][0]) / 2 -
 *     (C[0][2] + C[1][2]) / 2 (hind to front); ez = ex x ey.  All NaN when one of the six joints is missing or either squared
 *     length is at most 1e-18 of the largest squared norm of the six.
 * df3d_joint_angles: frame_dev holds nframes = 1 frame for all poses or nframes = T, one per pose (taken as given; a frame
 *     that holds a non-finite number makes its angles NaN).  Segment vectors are taken to leg coordinates (v.ex, s v.ey, v.ez),
 *     s = +1 on side 0 and -1 on side 1.  angles_dev [T, 6, 8] radians: thc_yaw, thc_pitch, thc_roll, ctr_pitch, ctr_roll,
 *     fti_pitch, fti_roll, tita_pitch (config.LEG_ANGLE_NAMES; definitions and NaN rules in DESIGN.md section 14); lengths_dev
 *     [T, 6, 4] = coxa, femur, tibia, tarsus, NaN where an end joint is missing (may be NULL).  Coordinates whose fourth
 *     powers overflow are outside the model.
 * n, T >= 0 (0: nothing to do, nothing is launched); outputs overlap neither an input nor each other, and angles_dev and
 *     lengths_dev are 16-byte aligned (they are written as 16-byte stores).
 *     Both asynchronous on `stream`; arguments are validated before the device is touched.
 * ---------------------------------------------------------------------------------------------- */
int df3d_body_frame(const double* pts_dev, long long n, double* frame_dev, void* stream);
int df3d_joint_angles(const double* pts_dev, long long T, const double* frame_dev, long long nframes, double* angles_dev,
                      double* lengths_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a11 constant-length legs fitted to the 3-D pose (the model is this project's own specification, defined
 *     in float64 by tests/leg_fit_oracle.py).  The reference stops at the pose.
 * pts_dev [T, 38, 3] float64 as in a10, with a10's legs and "missing joint" rule.  lengths_host [6, 4]: the fixed lengths
 *     (coxa, femur, tibia, tarsus) of every leg, finite and > 0.  anchor_host [6, 3] or NULL: where every leg starts; NULL
 *     anchors each leg at its own measured body-coxa joint.  Both are HOST arrays, read before the call returns.
 * Per (frame, leg): p0 = the anchor or the measured P0, targets t_k = P_k - p0 (k = 1..4), unknowns four unit directions d_i,
 *     chain c_k = sum_{i <= k} l_i d_i, cost E = sum_k |c_k - t_k|^2, minimised from the measured directions by a damped Newton
 *     method on the four spheres (tangent steps, an 8 x 8 Cholesky solve per trial, lambda from 0 in decades between 1e-3 and
 *     1e12, a step of at most 1e-9 in every tangent coordinate ends it; section 15 has every constant).
 * out_pts_dev [T, 38, 3]: the 30 leg joints, P0' = p0 and Pk' = p0 + c_k; the other eight joints are NOT written (the caller
 *     fills them).  May be pts_dev itself (in place); otherwise it must not overlap pts_dev.
 * cost_dev [T, 6]: the final E.  info_dev [T, 6, 2] int32, 8-byte aligned: (status, accepted iterations); status 0 = converged,
 *     1 = max_iter reached (max_iter = 0: the measured directions replayed with the fixed lengths), 2 = lambda passed 1e12.
 * A leg is not fitted -- its five joints are the input's bits, cost NaN, status -1, iterations -1 -- when one of P1..P4 is
 *     missing, when P0 is missing and no anchor is given, or when a measured segment's squared length is at most 1e-18 of the
 *     largest squared target.
 * DF3D_EINVAL before the device is touched: T < 0, max_iter < 0, a null pointer (only the anchor may be), a length that is not
 *     finite or not > 0, a non-finite anchor entry, out overlapping pts without being pts, cost or info overlapping anything,
 *     a misaligned info.  T = 0 launches nothing.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------- */
int df3d_leg_fit(const double* pts_dev, long long T, const double* lengths_host, const double* anchor_host, int max_iter,
                 double* out_pts_dev, double* cost_dev, int* info_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a12 Morlet wavelet spectrogram of a bundle of time series (the model is this project's own
 *     specification, defined in float64 by tests/spectrogram_oracle.py).  The reference stops at the pose.
 * The bank: F frequencies freqs_host [F] (Hz, a HOST array read before the call returns, ascending), the sampling rate fps, the
 *     wavelet's centre omega0 and the cut radius.  Row i: sigma_i = omega0 fps / (2 pi f_i) samples, K_i = ceil(radius sigma_i),
 *     and for k = -K_i..K_i: g = exp(-k^2 / (2 sigma_i^2)), phi = 2 pi f_i k / fps, kappa_i = sum g cos phi / sum g,
 *     n_i = 2 / sum g, a_i[k] = n_i g (cos phi - kappa_i), b_i[k] = -n_i g sin phi.
 * df3d_spectrogram_work_bytes: the bytes of the caller-owned DEVICE workspace that holds the bank's tap pairs (0 where the bank is
 *     refused).  df3d_spectrogram_bank fills it (one small kernel); df3d_spectrogram reads it and must be given the same bank.
 * x_dev [C, T] float64, channel-major.  out_dev [T, C, F], float64 (out_f32 = 0) or float32 (out_f32 = 1; accumulated in float64
 *     and rounded once): S[t, c, i] = sqrt(A^2 + B^2), A = sum_k a_i[k] x[c, clamp(t + k, 0, T - 1)], B likewise with b_i; NaN
 *     where A or B is not finite, that is where a sample in the support of (t, i) is not finite.
 * df3d_spectrogram_tile: the number of consecutive times one block owns (a test sweeps T around it).
 * DF3D_EINVAL before the device is touched, with a message that names the argument: T < 0, C < 1, F outside [1, 64]; fps,
 *     freqs[0] (f_min), omega0 or radius not finite and > 0; descending frequencies (f_max < f_min); f_max > fps / 2; a K_i above
 *     the cap of 2048 samples (the message gives the smallest f_min that fits); out_f32 other than 0 or 1; a null pointer; x not
 *     8-byte aligned, out not aligned to its element, work not 16-byte aligned; out overlapping x, work overlapping either; a
 *     workspace below df3d_spectrogram_work_bytes; more than 2^31 - 1 blocks.  T = 0 launches nothing (its pointers may be NULL).
 *     Both launching entries are asynchronous on `stream`; neither allocates nor keeps a host pointer.
 * ---------------------------------------------------------------------------------------------- */
int df3d_spectrogram_tile(void);
long long df3d_spectrogram_work_bytes(const double* freqs_host, int F, double fps, double omega0, double radius);
int df3d_spectrogram_bank(const double* freqs_host, int F, double fps, double omega0, double radius, void* work_dev,
                          long long work_len_bytes, void* stream);
int df3d_spectrogram(const double* x_dev, long long T, int C, const double* freqs_host, int F, double fps, double omega0,
                     double radius, const void* work_dev, long long work_len_bytes, void* out_dev, int out_f32, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a13 t-SNE behaviour map of per-frame spectra (the model is this project's own specification, defined
 *     in float64 by tests/behaviour_map_oracle.py).  All arrays are DEVICE float64 / int32, row-major; every stage is its own
 *     entry.  No floating-point atomics and fixed-order sums: two calls on the same input give the same bits.
 * df3d_bmap_prepare: S [T, D] -> p, logp [T, D], e [T], valid [T].  A row is valid when every entry is finite and >= 0 and its sum
 *     a is finite and > 0; then p = (S / a + floor) / (1 + D floor), logp = log p, e = sum_d p logp, valid = 1.  Otherwise p, logp
 *     and e are NaN and valid = 0.  df3d_bmap_logs: logp and e of distributions that exist already (positive entries).
 * df3d_bmap_divergence: K [M, N] = max(0, ea_i - sum_d pa[i, d] lb[j, d]), the Kullback-Leibler divergence of row i of one set
 *     (pa [M, D], ea [M]) from row j of another (lb [N, D], its LOGARITHMS).  At most 65 535 * 128 rows per call.
 * df3d_bmap_calibrate: per row of K [M, N], the conditional c[i, j] = exp(-beta_i (K[i, j] - m_i)) / sum_{j' != x_i} exp(...) with
 *     m_i the smallest admitted entry, c[i, x_i] = 0, x_i = exclude[i] (exclude NULL, or an entry of -1: no column excluded), and
 *     beta_i the root of H_i(beta) = -sum c log c = log(perplexity), accepted when |H_i - log perplexity| <= tol.  Where no beta in
 *     (0, beta_max] reaches the target (at least `perplexity` admitted entries tie at the minimum) beta_i = beta_max and bit 0 of
 *     info[i] is set; bit 1 reports a search that ran out of steps.  N <= 16 384 (the row stays in LDS).
 * df3d_bmap_joint: P [N, N] = (c + c^T) / (2N), zero diagonal.  df3d_bmap_place: out [M, 2] = c [M, N] Y [N, 2].
 * df3d_tsne_run: iterations first_iter .. first_iter + num_iters - 1 of the descent on Y, V, G [N, 2] (in place): alpha = 12,
 *     mu = 0.5 for an iteration index below 250, alpha = 1, mu = 0.8 from there; w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij,
 *     g_i = 4 sum_j (alpha P_ij - w_ij / Z) w_ij (y_i - y_j); per component G += 0.2 where g V < 0, else G *= 0.8, G = max(G, 0.01);
 *     V = mu V - lr G g; Y += V.  Two launches per iteration, no read-back: [0, k) followed by [k, n) gives the bits of [0, n).
 * df3d_bmap_cost: cost[0] = sum_{P_ij > 0} P_ij log(P_ij Z / w_ij).  df3d_bmap_work_bytes(N): the bytes of the caller-owned
 *     workspace of df3d_tsne_run and df3d_bmap_cost (0 where N is outside [1, 16 384]).
 * DF3D_EINVAL before the device is touched, with a message that names the argument: a negative count, D < 1, N outside its
 *     range, a null, misaligned (8 bytes; 16 for Y, out and work; 4 for int32) or overlapping buffer, a floor, tol, beta_max or lr
 *     that is not finite and positive (floor may be 0), a perplexity that is not finite or <= 1 or above n / 3 with n the number
 *     of admitted entries (the message gives the smallest frame count and the largest perplexity accepted), a workspace below
 *     the query, a block count that overflows.  An empty problem (T = 0, M = 0, num_iters = 0) launches nothing and returns
 *     DF3D_OK.  Every launching entry is asynchronous on `stream`, allocates nothing and keeps no host pointer.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_bmap_work_bytes(int N);
int df3d_bmap_prepare(const double* S_dev, long long T, int D, double floor_, double* p_dev, double* logp_dev, double* e_dev,
                      int* valid_dev, void* stream);
int df3d_bmap_logs(const double* p_dev, long long T, int D, double* logp_dev, double* e_dev, void* stream);
int df3d_bmap_divergence(const double* pa_dev, const double* ea_dev, long long M, const double* lb_dev, long long N, int D,
                         double* K_dev, void* stream);
int df3d_bmap_calibrate(const double* K_dev, long long M, int N, double perplexity, double tol, double beta_max, const int* exclude_dev,
                        double* cond_dev, double* beta_dev, int* info_dev, void* stream);
int df3d_bmap_joint(const double* cond_dev, int N, double* P_dev, void* stream);
int df3d_bmap_place(const double* cond_dev, long long M, int N, const double* Y_dev, double* out_dev, void* stream);
int df3d_bmap_cost(const double* P_dev, int N, const double* Y_dev, double* cost_dev, void* work_dev, long long work_len_bytes,
                   void* stream);
int df3d_tsne_run(const double* P_dev, int N, double* Y_dev, double* V_dev, double* G_dev, int first_iter, int num_iters, double lr,
                  void* work_dev, long long work_len_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a14 segmentation of the behaviour map (the model is this project's own specification, defined in float64
 *     by tests/behaviour_segment_oracle.py).  All arrays are DEVICE arrays, row-major: float64, int32, and int64 for the ethogram.
 *     No floating-point atomics and fixed-order sums: two calls on the same input give the same bits, on any machine.  A row of
 *     Y [T, 2] is valid when both entries are finite.
 * df3d_bseg_bounds: bounds[5] = min x, max x, min y, max y over the valid rows and their count M (a double; +-inf and 0 where
 *     there is none).
 * df3d_bseg_density: rho [G, G], rho[r, q] = (M 2 pi sigma^2)^-1 sum_valid t exp(-((gx_q - Y[t, 0])^2 + (gy_r - Y[t, 1])^2) / (2 sigma^2))
 *     with gx_q = x0 + (q + 0.5) h and gy_r = y0 + (r + 0.5) h: the exact sum over every valid frame, computed as the separable
 *     product on v_mfma_f64_16x16x4_f64 in slices of 2 048 frames that are added in index order.  All zeros where M = 0.
 * df3d_bseg_watershed: cells are ordered by the key (rho, -index), index = r G + q; a cell points at the 8-neighbour with the
 *     largest key if that key exceeds its own, else it is a root, and every cell's root is the end of its chain.  A root is kept
 *     when rho > 0 and rho >= min_peak max rho; kept roots are numbered 1 .. R by rising index.  regions [G, G]: the number of the
 *     cell's root, 0 where it was dropped.  num_regions[0] = R.  root_cells [G * G]: the kept roots' indices, then -1.  rho is
 *     finite and >= 0.
 * df3d_bseg_labels: labels [T] = -1 for an invalid row, else regions[r, q] with q = clamp(floor((Y[t, 0] - x0) / h), 0, G - 1) and r
 *     likewise from Y[t, 1] and y0.
 * df3d_bseg_bouts: the maximal runs of equal labels.  bouts [T, 3] int64: row b < B is (label, start, length), the rows from B on
 *     are zero; num_bouts[0] = B; occupancy [R + 1] int64: the frames of label 0 .. R; transitions [R + 1, R + 1] int64: the pairs
 *     (t, t + 1) whose labels are both in [0, R] and differ.  A label outside [-1, R] is counted in neither table.
 * df3d_bseg_work_bytes(T, G): the bytes of the caller-owned workspace that serves every entry above at this T and G (0 where T or
 *     G is out of range).
 * DF3D_EINVAL before the device is touched, with a message that names the argument: G outside [2, 1 024]; T negative or above
 *     65 535 * 2 048 (bounds, density) or 2^31 - 1 (labels, bouts); sigma, h, x0 or y0 not finite, sigma or h <= 0; min_peak outside
 *     [0, 1]; num_regions outside [0, 32 767]; a null, misaligned (16 bytes for Y and work, 8 for float64 and int64, 4 for int32) or
 *     overlapping buffer; a workspace below the query.  T = 0 launches nothing and returns DF3D_OK.  Every launching entry is
 *     asynchronous on `stream`, allocates nothing and keeps no host pointer.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_bseg_work_bytes(long long T, int G);
int df3d_bseg_bounds(const double* Y_dev, long long T, double* bounds_dev, void* stream);
int df3d_bseg_density(const double* Y_dev, long long T, double x0, double y0, double h, int G, double sigma, double* rho_dev, void* work_dev,
                      long long work_len_bytes, void* stream);
int df3d_bseg_watershed(const double* rho_dev, int G, double min_peak, int* regions_dev, int* num_regions_dev, int* root_cells_dev,
                        void* work_dev, long long work_len_bytes, void* stream);
int df3d_bseg_labels(const double* Y_dev, long long T, double x0, double y0, double h, int G, const int* regions_dev, int* labels_dev,
                     void* stream);
int df3d_bseg_bouts(const int* labels_dev, long long T, int num_regions, long long* bouts_dev, int* num_bouts_dev, long long* occupancy_dev,
                    long long* transitions_dev, void* work_dev, long long work_len_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a15 gait analysis of the leg tips (the model is this project's own specification, defined in float64 by
 *     tests/gait_oracle.py).  All arrays are DEVICE arrays, row-major: float64, int32, and int64 for steps and counts.  No
 *     floating-point atomics and fixed-order sums: two calls on the same input give the same bits, on any machine.  Leg L = 3 side +
 *     l, its joints P0 .. P4, the leg coordinates q(v) = (v . ex, +-v . ey, v . ez) (mirrored on side 1) and the missing-joint rule
 *     are those of df3d_joint_angles.
 * df3d_gait_velocity: pts [T, 38, 3] and the body frame(s) [nframes, 3, 3], nframes = 1 or T, as in df3d_joint_angles.  tip [T, 6, 3]
 *     = q(P4 - P0), NaN where P0 or P4 is missing or the frame holds a non-finite number.  vel [T, 6, 3] = q(P4[b] - P4[a]) (fps /
 *     (b - a)) with a = max(t - half_window, 0) and b = min(t + half_window, T - 1), in frame t's body frame; NaN where b = a, where
 *     P4 is missing at a or at b, or where the frame holds a non-finite number.
 * df3d_gait_states: states [T, 6] int32 from the anterior velocity u = vel[t, L, 0]: a sample is unknown where u is NaN, swing where
 *     u > on, stance where u < off and undecided otherwise; the state is that of the last decided sample at or before t, as -1
 *     (unknown), 0 (stance), 1 (swing), and -1 where there is none.
 * df3d_gait_steps: a lift-off is a frame t >= 1 with states 0 then 1, a touch-down the reverse; a step of a leg is a pair of
 *     consecutive lift-offs t0 < t2 with no unknown state in [t0, t2], and t1 the touch-down between them.  steps [3 T, 4] int64:
 *     row r < S is (L, t0, t1, t2), ordered by (L, t0); metrics [3 T, 3]: swing duration (t1 - t0) / fps, stance duration (t2 - t1) /
 *     fps and stride tip[t1, L, 0] - tip[t0, L, 0]; the rows from S on are zero; num_steps[0] = S.  A state other than 0 and 1 is
 *     unknown.
 * df3d_gait_phase: phase [T, 6] = (t - t0) / (t2 - t0) for the step with t0 <= t < t2, NaN outside every step.
 * df3d_gait_coupling: mean [6, 6, 2] = the mean of (cos, sin)(2 pi (phase_i - phase_j)) over the count [6, 6] (int64) frames where both
 *     phases are finite, NaN where there is none; summed in slices of 2 048 frames that are added in index order.
 * df3d_gait_patterns: pattern [T] int32 = the mask of the legs in swing (bit L), -1 where a leg is unknown; histogram [64] int64 =
 *     the frames of every mask; state_counts [6, 3] int64 = every leg's unknown, stance and swing frames.
 * df3d_gait_work_bytes(T): the bytes of the caller-owned workspace that serves every entry above at this T (0 where T is out of
 *     range).
 * DF3D_EINVAL before the device is touched, with a message that names the argument: T negative or above (2^31 - 1) / 6; fps not
 *     finite or <= 0; on or off not finite, or on <= off; half_window outside [1, 64]; nframes other than 1 or T; a null, misaligned
 *     (16 bytes for work, 8 for float64 and int64, 4 for int32) or overlapping buffer; a workspace below the query.  T = 0 launches
 *     nothing and returns DF3D_OK.  Every launching entry is asynchronous on `stream`, allocates nothing and keeps no host pointer.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_gait_work_bytes(long long T);
int df3d_gait_velocity(const double* pts_dev, long long T, const double* frame_dev, long long nframes, double fps, int half_window,
                       double* tip_dev, double* vel_dev, void* stream);
int df3d_gait_states(const double* vel_dev, long long T, double on, double off, int* states_dev, void* work_dev, long long work_len_bytes,
                     void* stream);
int df3d_gait_steps(const int* states_dev, const double* tip_dev, long long T, double fps, long long* steps_dev, double* metrics_dev,
                    int* num_steps_dev, void* work_dev, long long work_len_bytes, void* stream);
int df3d_gait_phase(const int* states_dev, long long T, double* phase_dev, void* work_dev, long long work_len_bytes, void* stream);
int df3d_gait_coupling(const double* phase_dev, long long T, double* mean_dev, long long* count_dev, void* work_dev, long long work_len_bytes,
                       void* stream);
int df3d_gait_patterns(const int* states_dev, long long T, int* pattern_dev, long long* histogram_dev, long long* state_counts_dev,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * a16 repair of the 3-D pose (the model is this project's own specification, defined in float64 by
 *     tests/pose_repair_oracle.py): a Hampel test of every joint, then linear filling of short gaps.  All arrays are DEVICE arrays,
 *     row-major.  pts [T, 38, 3] float64 in the layout of points3d_wo_procrustes; a joint is missing by df3d_joint_angles' rule (a
 *     non-finite coordinate, or all three exactly 0).  No floating-point atomics, no fused multiply-add: the outputs are the oracle's
 *     bits, and two calls give the same.
 * df3d_repair_outliers: flags [T, 38] uint8, bit 0 = missing, bit 1 = outlier.  For a joint that is not missing at t, V = the frames of
 *     [max(t - half_window, 0), min(t + half_window, T - 1)] where it is not missing, n = |V|.  n < min_count: untested (flags 0,
 *     score NaN).  Else per coordinate m = median over V, dev_s = |x_s - m|, mad = median of dev over V, thr = max(scale mad, floor);
 *     an outlier where dev_t > thr in any coordinate.  The median of an even count is the mean of the two middle values.  `scale` is
 *     the threshold times 1.4826, formed by the caller.  score [T, 38] float64 (may be null: not written) = the largest over the
 *     coordinates of dev_t / thr (0 where dev_t = 0, +inf where thr = 0 < dev_t), NaN for a missing or untested joint.  The test is
 *     not iterated.
 * df3d_repair_fill: a joint is bad where its flags are not 0.  With a the last good frame before t and b the first after it, the gap
 *     is filled when both exist and b - a - 1 <= max_gap: out = x_a + (x_b - x_a) ((t - a) / (b - a)); otherwise out = +0.0, which
 *     is missing.  Good joints keep their bits.  status [T, 38] int8: 0 kept, 1 missing and filled, 2 outlier and filled, 3 missing
 *     and left, 4 outlier and removed (bit 0 decides where both are set); counts [38, 5] int64: the frames per joint and code.
 * df3d_repair_work_bytes(T): the bytes of the caller-owned workspace of df3d_repair_fill at this T (0 where T is out of range).
 * DF3D_EINVAL before the device is touched, with a message that names the argument: T negative or above (2^31 - 1) / 38;
 *     half_window outside [1, 64]; scale not finite or <= 0; floor not finite or < 0; min_count outside [1, 2 half_window + 1];
 *     max_gap outside [0, 1000000]; a null (score excepted), misaligned (16 bytes for work, 8 for float64 and int64) or overlapping
 *     buffer; a workspace below the query.  T = 0 launches nothing and returns DF3D_OK.  Every launching entry is asynchronous on
 *     `stream`, allocates nothing and keeps no host pointer.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_repair_work_bytes(long long T);
int df3d_repair_outliers(const double* pts_dev, long long T, int half_window, double scale, double floor, int min_count,
                         unsigned char* flags_dev, double* score_dev, void* stream);
int df3d_repair_fill(const double* pts_dev, const unsigned char* flags_dev, long long T, int max_gap, double* out_dev,
                     signed char* status_dev, long long* counts_dev, void* work_dev, long long work_len_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a17 the treadmill ball and the fictive walking path from the stance tips (the model is this project's own
 *     specification, defined in float64 by tests/treadmill_oracle.py).  All arrays are DEVICE arrays, row-major: float64, int32 for
 *     states and legs, int64 for info and skipped.  No floating-point atomics and fixed-order sums: two calls on the same input give
 *     the same bits, on any machine.  The legs, the tip P4, the window and the missing-joint rule are those of a15.
 * df3d_ball_tips: pts [T, 38, 3], the recording's body frame [3, 3] (rows ex, ey, ez) and coxa [6, 3], the temporal medians of the six
 *     body-coxa joints; the origin o is their sum in leg order divided by 6.  tip [T, 6, 3] = F (P4 - o), neither mirrored nor relative
 *     to the coxa; NaN where P4 is missing or the frame or o holds a non-finite number.  vel [T, 6, 3] = F (P4[b] - P4[a]) (fps / (b -
 *     a)) with a15's window and NaN rules.
 * df3d_ball_fit: one sphere through the samples (t, L) with states 0 and a finite tip.  With m their mean and q = tip - m, the
 *     algebraic fit minimises sum (|q|^2 - 2 a . q - k)^2: centre a + m, radius sqrt(k + |a|^2).  known_radius = 1: the radius is
 *     `radius`, and the centre takes `iterations` Gauss-Newton steps on sum (|tip - c| - radius)^2 from the algebraic centre -- or,
 *     where there is none (three samples, a flat set), from m (1 + radius / |m|), the point beyond the tips as seen from the body's
 *     origin (status bit 1).  Refused (status bit 0; centre, radius and rms NaN): fewer than 4 samples (3 with a known radius), a
 *     Cholesky pivot at or below pivot_min times the largest diagonal entry of its normal matrix, or k + |a|^2 <= 0.  ball [8] =
 *     centre, radius, rms of |tip - c| - radius, and three zeros; info [2] int64 = count, status; sums [17] = the count, the sum of
 *     tip [3], and sum qx qx, qx qy, qx qz, qx, qy qy, qy qz, qy, qz qz, qz, qx |q|^2, qy |q|^2, qz |q|^2, |q|^2.  Every sum is
 *     taken in slices of 2 048 samples of the flattened [6 T] that are added in index order.
 * df3d_ball_rotation: per frame, over the legs with states 0 and finite tip and vel, r = tip - c: omega [T, 3] solves sum (|r|^2 I -
 *     r r^T) omega = sum r x vel, summed in leg order; NaN with fewer than min_legs legs, with a pivot at or below pivot_min times the
 *     trace, or with a refused ball.  legs [T] int32; residual [T] = the root mean square over those legs of |vel - omega x r|;
 *     fictive [T, 3] = (forward, sideways, yaw rate) = (s . ex, s . ey, -omega . u) with u = -c / |c| and s = -(omega x radius u).
 * df3d_ball_path: path [T, 3] = (x, y, theta), two exclusive prefix sums: theta of yaw / fps, then (x, y) of Rot(theta_t)(forward,
 *     sideways) / fps.  A frame with a non-finite fictive component moves nothing and is counted in skipped [1] int64.
 * df3d_ball_work_bytes(T): the bytes of the caller-owned workspace of df3d_ball_fit and df3d_ball_path at this T (0 where T is out of
 *     range).
 * DF3D_EINVAL before the device is touched, with a message that names the argument: T negative or above (2^31 - 1) / 6; fps not
 *     finite or <= 0; half_window outside [1, 64]; known_radius other than 0 or 1 and, with 1, a radius not finite or <= 0 or
 *     iterations outside [1, 64]; pivot_min outside [0, 1); min_legs outside [2, 6]; a null, misaligned (16 bytes for work, 8 for
 *     float64 and int64, 4 for int32) or overlapping buffer; a workspace below the query.  T = 0 launches nothing and returns DF3D_OK.
 *     Every launching entry is asynchronous on `stream`, allocates nothing and keeps no host pointer.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_ball_work_bytes(long long T);
int df3d_ball_tips(const double* pts_dev, long long T, const double* frame_dev, const double* coxa_dev, double fps, int half_window,
                   double* tip_dev, double* vel_dev, void* stream);
int df3d_ball_fit(const double* tip_dev, const int* states_dev, long long T, int known_radius, double radius, int iterations, double pivot_min,
                  double* ball_dev, long long* info_dev, double* sums_dev, void* work_dev, long long work_len_bytes, void* stream);
int df3d_ball_rotation(const double* tip_dev, const double* vel_dev, const int* states_dev, long long T, const double* ball_dev, int min_legs,
                       double pivot_min, double* omega_dev, int* legs_dev, double* residual_dev, double* fictive_dev, void* stream);
int df3d_ball_path(const double* fictive_dev, long long T, double fps, double* path_dev, long long* skipped_dev, void* work_dev,
                   long long work_len_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a18 tracking of the 2-D detections through time: an exact Viterbi solve over the heat-map peaks (the model is
 *     this project's own specification, defined in float64 / int64 by tests/track_oracle.py).  All arrays are DEVICE arrays, row-major,
 *     laid out as df3d_heatmap_peaks leaves them per camera: count [C, T, J] int32, pts [C, T, J, K, 2] float32 (row / H, col / W),
 *     val [C, T, J, K] float32.  A chain is one (camera, joint); the C J chains are independent.
 * df3d_track_peaks: slot k of a frame is valid when k < count and its value and both coordinates are finite; a frame without a valid
 *     slot is a placeholder frame: slot 0 alone is valid, its unary cost is 0 and every pair cost to or from it is w_motion.  Unary
 *     cost u = w_value min(v_best - v, 1) with v_best the largest valid value of the frame; pair cost d = w_motion min(dr^2 + dc^2,
 *     tau^2) / tau^2 between slot k of frame t and slot k' of frame t - 1, dr and dc the pixel differences (normalised x height_px, x
 *     width_px).  Both are formed in float64 in that order, without contraction, and rounded once: rint(x 2^20) as int64; an invalid
 *     slot costs 2^61, where sums saturate.  choice [C, T, J] int32 minimises the sum of u over the frames and d over the frames after
 *     the first; among the optimal paths it is the one whose reversed sequence is lexicographically smallest (the last frame takes
 *     the lowest minimal slot, every back-pointer the lowest minimising predecessor); 0 on a placeholder frame.  cost [C, J] int64:
 *     the minimum, in units of 2^-20.  The recurrence runs in blocks of block_frames frames, which changes no bit of either output.
 *     No atomics: two calls on the same input give the same bits.
 * df3d_track_work_bytes(nchain, T, K, block_frames): the bytes of the caller-owned workspace at nchain = C J chains (0 where an
 *     argument is out of range): 2 193 bytes per chain and block and 16 per chain and frame, each part rounded up to 64.
 * DF3D_EINVAL before the device is touched, with a message that names the argument: C or J below 1 or C J above 2^20; T negative,
 *     above 2^31 - 1 or C J T above 2^36; K outside [1, 16]; height_px, width_px or tau not finite or <= 0; w_motion or w_value not
 *     finite or outside [0, 1024]; block_frames outside [1, 4096]; T (w_motion + w_value) 2^20 at or above 2^60; more than 2^31 - 1
 *     (chain, block) pairs; a workspace below the query; a null, misaligned (16 bytes for work, 8 for cost, 4 for the rest) or
 *     overlapping buffer.  T = 0 launches nothing and returns DF3D_OK.  Asynchronous on `stream`, allocates nothing and keeps no
 *     host pointer.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_track_work_bytes(long long nchain, long long T, int K, int block_frames);
int df3d_track_peaks(const int* count_dev, const float* pts_dev, const float* val_dev, int C, long long T, int J, int K, double height_px,
                     double width_px, double tau, double w_motion, double w_value, int block_frames, int* choice_dev, long long* cost_dev,
                     void* work_dev, long long work_len_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a19 consensus triangulation over camera subsets (the model is this project's own specification, stated in
 *     float64 numpy by tests/consensus_oracle.py).  P_host [ncam, 3, 4] HOST float64 (pixels, no distortion: the DLT's model),
 *     pts_px_dev [ncam, T, J, 2] (row_px, col_px), X_full_dev [T, J, 3] = df3d_triangulate of the same detections (the all-views
 *     candidate is taken from it, not recomputed).  Per point (t, j): a camera is a view when both coordinates are non-zero (a6);
 *     every subset S of the views with |S| >= max(min_views, 2) is a candidate; X_S is its DLT (the views' 4x4 contributions added in
 *     ascending camera order, the a6 solve); camera c's error against a point is e = sqrt(q), q = du du + dv dv, du = u / w - col,
 *     dv = v / w - row, [u, v, w] = P_c [X; 1] in left-to-right sums, e = +inf when w > 0 fails or e is not finite.  S qualifies
 *     when every c in S has a finite e <= tau[j].  Chosen: the largest qualifying |S|, then the smaller sum of q over S (ascending
 *     camera order from 0.0), then the smaller bitmask.
 * df3d_triangulate_consensus: status_dev [T, J] int8: 0 = fewer than two views (X = 0, cameras = 0), 1 = the all-views set qualified
 *     (X = X_full), 2 = a proper subset was chosen (X = X_S), 3 = no subset qualified (X = X_full, cameras = all views).  X_dev
 *     [T, J, 3]; cameras_dev [T, J] int32, bit c set for each camera used; err_dev [ncam, T, J]: every view's e against the chosen X,
 *     rejected views included, 0 for non-views and at status 0; fixed_px_dev [ncam, T, J, 2] (may be NULL): the input detections with
 *     every rejected view (a view outside the chosen set) replaced by (v / w, u / w) of the chosen X; counts_dev [J, 4] int64 (may be
 *     NULL): how often each status occurred per joint, counted in slices of 256 frames added in index order.  tau_host [J] HOST
 *     float64, each >= 0 and not NaN (+inf accepts every finite error).  One launch for the points, two small ones for the counts;
 *     the candidates are never stored.  No atomics: two calls on the same input give the same bits.
 * df3d_consensus_candidates: every candidate of min_views = 2, indexed by camera bitmask: cand_X_dev [T, J, 2^ncam, 3] and
 *     cand_q_dev [T, J, 2^ncam, ncam] (q of the cameras in the candidate, +inf where e is); entries that belong to no candidate are
 *     0, the all-views entry holds X_full.  The candidate code is the fused entry's own; it exists so that the choice can be tested
 *     against an oracle that is given the device's candidate points.
 * df3d_consensus_work_bytes(ncam, T, J): the bytes of work_dev (0 where an argument is out of range): 32 J per slice of 256 frames.
 * 1 <= ncam <= 8, 1 <= J <= 64, T >= 0 (T = 0 launches nothing and returns DF3D_OK), 2 <= min_views <= 8.  DF3D_EINVAL before the
 *     device is touched, with a message, for a value outside those ranges, a bad tau, a workspace below the query, a null,
 *     misaligned (8 bytes for float64 / int64, 4 for cameras) or overlapping buffer.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_consensus_work_bytes(int ncam, int T, int J);
int df3d_consensus_candidates(const double* P_host, const double* pts_px_dev, const double* X_full_dev, int ncam, int T, int J,
                              double* cand_X_dev, double* cand_q_dev, void* stream);
int df3d_triangulate_consensus(const double* P_host, const double* pts_px_dev, const double* X_full_dev, int ncam, int T, int J,
                               const double* tau_host, int min_views, double* X_dev, int* cameras_dev, signed char* status_dev,
                               double* err_dev, double* fixed_px_dev, long long* counts_dev, void* work_dev, long long work_bytes,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * a20 trajectory triangulation (the model is this project's own specification, stated in float64 numpy by
 *     tests/trajectory_oracle.py, whose header lists every operation).  P_host [ncam, 3, 4] HOST float64; pts_px_dev [ncam, T, J, 2]
 *     (row_px, col_px); a camera is a view of (t, j) when both coordinates are non-zero (a6).  Per joint j (a chain) the points
 *     X[0 .. T - 1] minimise  sum over frames and views of huber_delta(e) + lambda[j] sum |X[t - 1] - 2 X[t] + X[t + 1]|^2,  e the
 *     reprojection error of a19, huber(e) = e e for e <= delta, else 2 delta e - delta delta; a view with w > 0 false or a non-finite
 *     error has weight 0.  An anchor is a frame with at least two views and a finite X0; the unknowns (the active frames) are the
 *     anchors and the frames between two anchors at most max_gap frames apart, where at least three such frames are consecutive;
 *     every other frame keeps the bits of X0.  Damped Gauss-Newton with IRLS weights (1, or delta / e beyond delta), one damping and
 *     one accept / reject decision per chain.
 * df3d_trajectory_linearize: at X_dev [T, J, 3], every frame: H_dev [T, J, 6] (sum of weight J^T J over the valid views in ascending
 *     camera order; entries 00 01 02 11 12 22), g_dev [T, J, 3] (sum of weight J^T r), weight_dev and err_dev [ncam, T, J] (0 for a
 *     non-view; an invalid view has weight 0 and error +inf), cost_dev [J] (the sum of the frames' huber terms in the model's fixed
 *     order: lane k adds the frames k, k + 256, ...; the 256 partial sums are halved 128, 64, ... 1).  work_dev: 8 T J bytes.
 * df3d_trajectory_solve: d_dev [T, J, 3] = -(H + lambda K + mu I)^-1 g on the frames where segment_dev [T, J] (int8) is non-zero, 0
 *     elsewhere; K is the Gram matrix of the second differences over the triples of consecutive non-zero frames, times I3; g_dev is
 *     the whole gradient.  The chain is cut into blocks of min(block_frames, max(T, 3)) frames, each lane eliminates its block's
 *     interior, the separators (the last two frames of every block) are solved as one banded system, the interiors are substituted
 *     back; block_frames >= T is the serial factorisation.  ok_dev [J] int32: 1 when every pivot was > 0.  ticks_dev [J, 4] int64 (may be NULL): the
 *     device's wall clock after the assembly, the interiors, the separators and the substitution of each chain, for
 *     tests/perf/bench_trajectory.py.
 * df3d_triangulate_trajectory: the whole fit from X0_dev [T, J, 3] (df3d_triangulate of the same detections), one persistent workgroup
 *     per chain.  X_dev [T, J, 3]; status_dev [T, J] int8: 0 not active (copied), 1 anchor, 2 filled frame with at least one view, 3
 *     filled frame without a view, 4 active frame of a chain that did not converge (the last accepted iterate); weight_dev, err_dev
 *     [ncam, T, J] at the final X (0 where the frame is not active); iterations_dev [J] int32 (accepted trials); cost_dev [J, 2]
 *     (start, final); counts_dev [J, 5] int64.  lambda_host [J] HOST float64, px^2 / mm^2, each >= 0 and finite; delta >= 0, not NaN
 *     (+inf: plain least squares).
 * df3d_trajectory_work_bytes(ncam, T, J, block_frames): the bytes of work_dev for the fit and the solve (0 where an argument is out
 *     of range, and for T = 0).
 * 1 <= ncam <= 8, 1 <= J <= 64, 0 <= T <= 1048576 (T = 0 launches nothing and returns DF3D_OK), 3 <= block_frames <= 1048576,
 *     0 <= max_gap <= 1000000, 0 <= mu <= 1e13.  DF3D_EINVAL before the device is touched, with a message, for a value outside those
 *     ranges, a bad lambda or delta, a workspace below the query, a null, misaligned (8 bytes for float64 / int64, 4 for int32) or
 *     overlapping buffer.  No atomics: two calls on the same input give the same bits.  Asynchronous on `stream`.
 *     A chain's whole iteration is one workgroup's launch: 0.11 s per 1 000 frames and 1.1 s per 20 000 on an MI355X at the fly layout
 *     (the slowest chain's 128 and 151 iterations); longer recordings were not measured, and 2^20 frames would run for about a minute.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_trajectory_work_bytes(int ncam, int T, int J, int block_frames);
int df3d_trajectory_linearize(const double* P_host, const double* pts_px_dev, const double* X_dev, int ncam, int T, int J, double delta,
                              double* H_dev, double* g_dev, double* weight_dev, double* err_dev, double* cost_dev, void* work_dev,
                              long long work_bytes, void* stream);
int df3d_trajectory_solve(const double* H_dev, const double* g_dev, const signed char* segment_dev, int T, int J, const double* lambda_host,
                          double mu, int block_frames, double* d_dev, int* ok_dev, long long* ticks_dev, void* work_dev, long long work_bytes,
                          void* stream);
int df3d_triangulate_trajectory(const double* P_host, const double* pts_px_dev, const double* X0_dev, int ncam, int T, int J,
                                const double* lambda_host, double delta, int max_gap, int block_frames, double* X_dev,
                                signed char* status_dev, double* weight_dev, double* err_dev, int* iterations_dev, double* cost_dev,
                                long long* counts_dev, void* work_dev, long long work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a21 heat-map triangulation (the model is this project's own specification, stated in float64 numpy by
 *     tests/heatmap3d_oracle.py, whose header lists every operation).  hm_dev [n, V, C, H, W] float32: the heat-maps of n frames and V
 *     views as the network saw them; P_host [V, 3, 4] HOST float64 (pixels); flip_host [V] HOST bytes (non-zero: the network saw the
 *     view mirrored); plane_host [V, J] HOST int32: the plane of joint j in view v, or -1.  cell_rows, cell_cols: the pixels of one
 *     heat-map cell (image rows / H, image columns / W); log_floor = log(floor), taken by the caller: a cell is log(h) where that lies
 *     above log_floor and h is finite, else log_floor.  The score of a 3-D point is the sum over the joint's views, ascending, of
 *     max(Catmull-Rom sample of the cells at the point's projection, log_floor) where w > 0 and the projection lies inside the plane
 *     (0 <= row <= H - 1, 0 <= column <= W - 1 in cells), else of log_floor.
 * df3d_heatmap3d_scores: out_dev [n, J, M] = the score of pts_dev [n, J, M, 3].  For tests: the sampler alone.
 * df3d_triangulate_heatmaps: from X0_dev [n, J, 3], `levels` levels of 8 x 8 x 8 points centre + (i - 3.5) step, step = 2 half / 8,
 *     index (ix 8 + iy) 8 + iz; the best is the largest score, ties to the lowest index, and the next level searches centre = that
 *     point, half = step.  X_dev [n, J, 3]; score_dev [n, J] (the last level's best; NaN for status 0); status_dev [n, J] int8: 0 fewer
 *     than two views, X0 not finite or X0 = (0, 0, 0): the bits of X0; 1 searched; 2 no point of level 0 scored above the all-floor
 *     score: X0; 3 searched, and the best point of level 0 lay on a face of its cube; views_dev [n, J] int32 (bit v: view v has a
 *     plane); shift_dev [n, J] = |X - X0|; choice_dev [n, J, levels] int32 (the index chosen at every level, -1 where none was);
 *     counts_dev [J, 4] int64; path_dev [n, J] int8 (may be NULL): 0 not searched, 1 the windows were staged in LDS, 2 they were not.
 *     One workgroup per (frame, joint) stages the logarithms of the cells its search can reach in LDS when they are at most `budget`
 *     doubles (0 <= budget <= df3d_heatmap3d_window_doubles(); 0 stages nothing); otherwise every tap reads the plane and takes the
 *     logarithm itself.  Both routes give the same bits.
 * 0 <= n <= 1048576 (n = 0 launches nothing and returns DF3D_OK), 1 <= V <= 8, 1 <= C <= 1024, 4 <= H, W <= 1024, 1 <= J <= 64,
 *     0 <= M <= 1048576, 1 <= levels <= 6, half finite and > 0, log_floor finite and < 0, plane indices in [-1, C).  DF3D_EINVAL before
 *     the device is touched, with a message, for a value outside those ranges, a null, misaligned (8 bytes for float64 / int64, 4
 *     for float32 / int32) or overlapping buffer.  No atomics: two calls on the same input give the same bits.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------- */
int df3d_heatmap3d_window_doubles(void);
int df3d_heatmap3d_scores(const float* hm_dev, int n, int V, int C, int H, int W, const double* P_host, const unsigned char* flip_host,
                          const int* plane_host, int J, const double* pts_dev, int M, double cell_rows, double cell_cols, double log_floor,
                          double* out_dev, void* stream);
int df3d_triangulate_heatmaps(const float* hm_dev, int n, int V, int C, int H, int W, const double* P_host, const unsigned char* flip_host,
                              const int* plane_host, int J, const double* X0_dev, double half, int levels, double cell_rows,
                              double cell_cols, double log_floor, int budget, double* X_dev, double* score_dev, signed char* status_dev,
                              int* views_dev, double* shift_dev, int* choice_dev, long long* counts_dev, signed char* path_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a23 per-camera frame lags from epipolar consistency (the model is this project's own specification, stated in
 *     numpy / int64 by tests/sync_oracle.py).  pts_px_dev [ncam, T, J, 2] (row_px, col_px); pairs_host [npair, 2] HOST int32, cameras
 *     a < b; F_host [npair, 9] HOST float64, row-major, x_b^T F x_a = 0 with x = (col_px, row_px, 1).  Lag d in [-D, D] pairs camera
 *     a's frame t with camera b's frame t + d for every joint; the sample is valid when neither detection has a zero coordinate and
 *     0 <= t + d < T.  l = F x_a, m = F^T x_b, s = x_b . l, e = s s / (l0 l0 + l1 l1 + m0 m0 + m1 m1), every sum left to right and every
 *     product rounded on its own; a sample whose denominator is 0 is skipped; its cost is q = floor(min(e, tau tau) 2^10 + 0.5) as
 *     int64 (a NaN costs tau tau).  The window of a sample is t / W, nW = ceil(T / W).
 * df3d_sync_pair_costs: cost_dev, count_dev [npair, nW, 2 D + 1] int64: the sum of q and the number of valid samples; index d + D.
 * df3d_sync_paths: per pair the lags d_0 .. d_{nW - 1} that minimise sum cost[w, d_w] + switch_q sum |d_w - d_{w - 1}|, an exact
 *     Viterbi on int64; ties, for a predecessor and for the last state, go to the smaller (|d|, d).  lag_dev [npair, nW] int32;
 *     path_cost_dev [npair] int64 (the minimum); margin_dev [npair, nW] float64, px^2: the smallest cost / count / 2^10 over the lags
 *     d != d_w with a sample, minus that of d_w (+inf where no other lag has one); NaN where the count at d_w is 0 or below
 *     min_count.  work_dev: df3d_sync_work_bytes(npair, nW, D) bytes (a byte per window and state; 0 for arguments out of range).
 * df3d_sync_apply: out_dev [ncam, T, J, 2]: camera c's frame t + lag_cam[c, t / W], zeros where that frame does not exist.
 *     lag_cam_dev [ncam, nW] int32 on the device.
 * 1 <= ncam <= 8, 1 <= J <= 64, 0 <= T <= 1048576, 0 <= npair <= 28, 0 <= D <= 64, W >= 1, 0 <= tau <= 4096, 0 <= switch_q <= 2^34,
 *     min_count >= 0: within them no sum leaves int64.  T = 0 and npair = 0 launch nothing and return DF3D_OK.  DF3D_EINVAL before the
 *     device is touched, with a message, for a value outside those ranges, a pair that is not 0 <= a < b < ncam, a workspace below
 *     the query, a null, misaligned (8 bytes for float64 / int64, 4 for int32) or overlapping buffer.  No atomics: two calls on the
 *     same input give the same bits.  Asynchronous on `stream`; the host arrays are copied before the call returns.
 * ---------------------------------------------------------------------------------------------- */
long long df3d_sync_work_bytes(int npair, long long nW, int D);
int df3d_sync_pair_costs(const double* F_host, const int* pairs_host, int npair, const double* pts_px_dev, int ncam, int T, int J, int D,
                         int W, double tau, long long* cost_dev, long long* count_dev, void* stream);
int df3d_sync_paths(const long long* cost_dev, const long long* count_dev, int npair, long long nW, int D, long long switch_q,
                    long long min_count, int* lag_dev, long long* path_cost_dev, double* margin_dev, void* work_dev, long long work_bytes,
                    void* stream);
int df3d_sync_apply(const double* pts_px_dev, const int* lag_cam_dev, int ncam, int T, int J, int W, double* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a7  bundle adjustment building blocks.   Replaces the arithmetic under pyba
 *     CameraNetwork.bundle_adjust(update_intrinsic=False, update_distort=False)
 *     (call site reference df3d/core.py:249).  Unknowns x = [ncam x (rvec, tvec)] ++ [npts x XYZ];
 *     observation i links camera cam_idx[i] to point pt_idx[i]; observations of one point are
 *     contiguous: point p owns observations [pt_start[p], pt_start[p+1]).
 * All arrays are device float64 / int32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct df3d_ba_problem {
    int ncam;              /* <= 8                                                        */
    int nobs;              /* number of 2-D observations (residual vector has 2*nobs)     */
    int npts;              /* number of 3-D points                                        */
    const double* intr4;   /* [ncam, 4]  fx, fy, cx, cy                                   */
    const double* obs_xy;  /* [nobs, 2]  x = col_px, y = row_px                           */
    const int* cam_idx;    /* [nobs]                                                      */
    const int* pt_idx;     /* [nobs]                                                      */
    const int* pt_start;   /* [npts + 1]  observations of point p: [pt_start[p], pt_start[p+1]) */
    const int* cam_perm;   /* [nobs]      observation ids grouped by camera (stable order)      */
    const int* cam_start;  /* [ncam + 1]  camera c owns cam_perm[cam_start[c] : cam_start[c+1]] */
} df3d_ba_problem;

/* Jacobian storage is component-major so per-observation threads read/write coalesced:
 *   Jc_dev [12, nobs]  entry (row*6 + col, i) = d r[2i+row] / d cam(cam_idx[i])[col]   (rvec 0..2, tvec 3..5)
 *   Jp_dev [ 6, nobs]  entry (row*3 + col, i) = d r[2i+row] / d point(pt_idx[i])[col]
 * scratch_dev arguments need DF3D_BA_SCRATCH_DOUBLES doubles; reductions run in a fixed order, so
 * results are bit-reproducible run to run. */
#define DF3D_BA_SCRATCH_DOUBLES 4096

/* residuals r[2*nobs] (interleaved x0,y0,x1,y1,...) and analytic Jacobian blocks at x; any of
 * r_dev / Jc_dev / Jp_dev may be NULL to skip it (Jc and Jp go together). */
int df3d_ba_eval(const df3d_ba_problem* p, const double* x_dev, double* r_dev, double* Jc_dev, double* Jp_dev,
                 void* stream);
/* colsq[n] = sum over rows of J[:, k]^2  (for scipy's x_scale='jac').  n = 6*ncam + 3*npts */
int df3d_ba_colsq(const df3d_ba_problem* p, const double* Jc_dev, const double* Jp_dev, double* colsq_dev,
                  double* scratch_dev, void* stream);
/* y[2*nobs] = J * (d .* v)      (d_dev may be NULL = ones) */
int df3d_ba_matvec(const df3d_ba_problem* p, const double* Jc_dev, const double* Jp_dev, const double* d_dev,
                   const double* v_dev, double* y_dev, void* stream);
/* w[n] = d .* (J^T u)           (d_dev may be NULL = ones) */
int df3d_ba_rmatvec(const df3d_ba_problem* p, const double* Jc_dev, const double* Jp_dev, const double* d_dev,
                    const double* u_dev, double* w_dev, double* scratch_dev, void* stream);

/* LSMR on A = J*diag(d) with Tikhonov `damp`, the inner solve of scipy's TRF (tr_solver='lsmr').
 * Synchronous: returns when the solve has stopped; x_dev[n] receives the solution.  Every scalar of the recurrence lives on the device.
 * work_dev: at least df3d_ba_lsmr_work_doubles(p) doubles (includes the scratch).  info_host[8] =
 * {istop, itn, normr, normar, normA, condA, normx, fallback} (fallback: 0, or why a persistent form handed the run to the launch-based
 * one: 1 its workgroups never became co-resident, 2 the problem does not fit it).
 * Forms (df3d_ba_lsmr_form; df3d_ba_lsmr = DF3D_LSMR_AUTO, the environment variable DF3D_LSMR_KERNELS = 0 | 1 | 2 | 11 overrides AUTO).
 * The values below are the only numbering: AUTO is resolved once per call (csrc/ba.hip: resolve_form), every other value names the code
 * that runs (lsmr_run), and one rule (lsmr_run_or_launches) repeats as LAUNCHES a run that LOCAL or BARRIERS could not take:
 *   DF3D_LSMR_LOCAL     ONE persistent kernel per solve: every workgroup owns a range of points with their observations, Jacobian slice and
 *                       vectors in registers, two small all-reduces per iteration, one read-back per solve.  Up to 128 ranges of
 *                       1 024 observations (every window of <= 1 000 frames); wants the device to itself: up to 128 workgroups of 512
 *                       threads and 96 KB of LDS have to be resident at once.  Sums grouped per range: last-bit differences from the others.
 *   DF3D_LSMR_LAUNCHES  two kernels per iteration, 16 iterations per host read-back: needs no co-residency -- the form to use
 *                       when the solve runs BESIDE other work on the device (a re-calibration next to the frame pipeline).
 *   DF3D_LSMR_BARRIERS  the launch-based arithmetic in one persistent kernel with grid-wide barriers (measured slower than
 *                       LAUNCHES: profiles/r05_ba_timings.txt);  DF3D_LSMR_ELEVEN  eleven kernels per iteration, the arithmetic reference.
 *                       LAUNCHES, BARRIERS and ELEVEN produce the same bits.
 *   DF3D_LSMR_AUTO      LOCAL where the problem fits, else LAUNCHES. */
#define DF3D_LSMR_AUTO 0
#define DF3D_LSMR_BARRIERS 1
#define DF3D_LSMR_LAUNCHES 2
#define DF3D_LSMR_LOCAL 3
#define DF3D_LSMR_ELEVEN 11
size_t df3d_ba_lsmr_work_doubles(const df3d_ba_problem* p);
int df3d_ba_lsmr(const df3d_ba_problem* p, const double* Jc_dev, const double* Jp_dev, const double* d_dev,
                 const double* b_dev, double damp, double atol, double btol, double conlim, int maxiter,
                 double* x_dev, double* work_dev, double* info_host, void* stream);
int df3d_ba_lsmr_form(const df3d_ba_problem* p, const double* Jc_dev, const double* Jp_dev, const double* d_dev,
                      const double* b_dev, double damp, double atol, double btol, double conlim, int maxiter,
                      double* x_dev, double* work_dev, double* info_host, void* stream, int form);

/* small device-vector helpers used by the host TRF driver (all float64, asynchronous except dot) */
int df3d_vec_dot(const double* a_dev, const double* b_dev, size_t n, double* result_host, double* scratch_dev,
                 void* stream); /* synchronous; scratch_dev >= 1024 doubles */
/* `count` (1..8) dot products a_dev[j] . b_dev[j] of lengths n[j] in ONE launch and ONE synchronising read-back (results_host[count]); every
 * product is summed exactly as df3d_vec_dot sums it (same grid, same order: the same bits).  The trust-region driver of a7 needs its
 * scalars in groups (the 2 x 2 subspace system: five products) -- round 4, reference call site df3d/core.py:249.
 * scratch_dev: DF3D_BA_SCRATCH_DOUBLES doubles. */
int df3d_vec_dots(int count, const double* const* a_dev, const double* const* b_dev, const size_t* n, double* results_host,
                  double* scratch_dev, void* stream); /* synchronous; scratch_dev >= DF3D_BA_SCRATCH_DOUBLES (uses 8*256+8) */
int df3d_vec_axpby(double a, const double* x_dev, double b, const double* y_dev, double* out_dev, size_t n,
                   void* stream); /* out = a*x + b*y (y may be NULL)        */
int df3d_vec_mul(const double* x_dev, const double* y_dev, double* out_dev, size_t n, void* stream);
int df3d_vec_absmax(const double* a_dev, size_t n, double* result_host, double* scratch_dev, void* stream); /* sync */
/* sum over npairs (x, y) pairs of sqrt(x^2 + y^2): with the residuals of df3d_ba_eval this is nobs x the mean
 * re-projection distance in pixels that CameraNetwork.reprojection_error() reports (call site reference
 * df3d/core.py:250); fixed summation order; synchronises like df3d_vec_dot */
int df3d_vec_pairnorm_sum(const double* r_dev, size_t npairs, double* result_host, double* scratch_dev, void* stream);
/* scipy's x_scale='jac': scale_inv = sqrt(colsq) (0 -> 1 when first != 0, else max with the previous value),
 * scale = 1 / scale_inv */
int df3d_ba_update_scale(const double* colsq_dev, double* scale_inv_dev, double* scale_dev, size_t n, int first,
                         void* stream);

/* The trust-region driver with its scalars on the device (round 6): what deepfly3d_amd/bundle_adjust.py:solve_trf does between two
 * evaluations, as three calls with ONE stream synchronisation each instead of one per scalar group.  They replace the solver loop of
 * scipy.optimize.least_squares(method='trf', tr_solver='lsmr', x_scale='jac') that pyba runs (reference call site df3d/core.py:249);
 * the arithmetic is that of the separate calls above, operation for operation (same kernels, same fixed summation orders).
 * All vectors are device float64: n = 6 ncam + 3 npts columns, m = 2 nobs rows; scratch_dev: DF3D_BA_SCRATCH_DOUBLES; work_dev:
 * df3d_ba_lsmr_work_doubles(p).
 * df3d_ba_trf_subspace: from (J, scale, g = J^T f, f, Delta): |g|_inf, g_h = scale g, the damping of the 1-D Cauchy model, the LSMR step
 *   gn_h (damping read from device memory by the data-local form; the other forms take one more read-back), the orthonormal basis
 *   S = [s0 s1] of span{g_h, gn_h} (LAPACK's QR signs), J_h S and the 2x2 model.  out_host[19]: |g|_inf, |J_h g_h|^2, |g_h|^2, damp, r01,
 *   |s1|^2 (before normalisation), B_S[0][0], B_S[0][1], B_S[1][1], g_S[0], g_S[1], then df3d_ba_lsmr's info[8].
 *   When gn_h is parallel to g_h to rounding (|s1| < 2^-20 |r01|: an LSMR run that one iteration ends) s1 takes a second Gram-Schmidt
 *   pass against s0, with two more read-backs; r01 and |s1|^2 are reported as the first pass left them.
 * df3d_ba_trf_trial: step_h = p0 s0 + p1 s1, x_new = x + scale step_h, f_new = residuals(x_new); out_host[6]: |J_h step_h|^2, step_h . g_h,
 *   |step_h|^2, |f_new|^2, |step|^2, |x|^2.
 * df3d_ba_trf_linearize: J (and f when eval_f != 0) at x, g = J^T f, x_scale='jac' bookkeeping (first != 0: the first call); no read-back. */
int df3d_ba_trf_subspace(const df3d_ba_problem* p, const double* Jc_dev, const double* Jp_dev, const double* scale_dev, const double* g_dev,
                         const double* f_dev, double Delta, double* g_h_dev, double* gn_h_dev, double* s0_dev, double* s1_dev, double* Js0_dev,
                         double* Js1_dev, double* tmp_m_dev, double* work_dev, double* scratch_dev, double* out_host, void* stream, int form);
int df3d_ba_trf_trial(const df3d_ba_problem* p, double p0, double p1, const double* s0_dev, const double* s1_dev, const double* Js0_dev,
                      const double* Js1_dev, const double* scale_dev, const double* x_dev, const double* g_h_dev, double* step_h_dev,
                      double* tmp_m_dev, double* step_dev, double* x_new_dev, double* f_new_dev, double* scratch_dev, double* out_host, void* stream);
int df3d_ba_trf_linearize(const df3d_ba_problem* p, const double* x_dev, double* f_dev, int eval_f, double* Jc_dev, double* Jp_dev, double* g_dev,
                          double* colsq_dev, double* scale_inv_dev, double* scale_dev, int first, double* scratch_dev, void* stream);

/* Robust losses for the adjustment, with the semantics of scipy.optimize.least_squares(method='trf', loss=..., f_scale=...) (an opt-in
 * beside the reference's plain sum of squares, call site reference df3d/core.py:249).  With C = f_scale and z = (f / C)^2 PER SCALAR residual:
 *   cost = 1/2 C^2 sum rho(z),   w = rho'(z),   s^2 = rho' + 2 z rho'' clamped below at 2^-52;   J's row times s, f <- f w / s.
 *   soft_l1: rho = 2 (sqrt(1 + z) - 1)   huber: z (z <= 1), 2 sqrt(z) - 1   cauchy: log1p(z)   arctan: atan(z)   linear: z (w = s = 1)
 * The scaled (J, f) go through every entry above unchanged (matvec, rmatvec, colsq, every LSMR form, df3d_ba_trf_subspace).
 * Every entry refuses an unknown loss, an f_scale that is not positive and finite, and null pointers before it touches the device.
 * df3d_ba_eval_robust: one pass, one lane per observation as df3d_ba_eval: the scaled f (f_dev[2 nobs], required), the scaled Jc / Jp rows
 *   (NULL together to skip), and optionally the unscaled residuals (f_true_dev[2 nobs]) and the weights (w_dev[2 nobs]).
 * df3d_ba_robust_cost: 1/2 C^2 sum rho over a vector of m UNSCALED residuals, summed in df3d_vec_dot's order (a residual that is not
 *   finite gives NaN); synchronous.
 * df3d_ba_trf_linearize_robust / df3d_ba_trf_trial_robust: df3d_ba_trf_linearize / df3d_ba_trf_trial for a robust loss.  linearize always
 *   evaluates f (scaled into f_dev; f_true_dev and w_dev optional); trial leaves the UNSCALED residuals in f_new_dev and returns the robust
 *   cost in out_host[3], where df3d_ba_trf_trial returns |f_new|^2. */
#define DF3D_BA_LOSS_LINEAR 0
#define DF3D_BA_LOSS_SOFT_L1 1
#define DF3D_BA_LOSS_HUBER 2
#define DF3D_BA_LOSS_CAUCHY 3
#define DF3D_BA_LOSS_ARCTAN 4
int df3d_ba_eval_robust(const df3d_ba_problem* p, const double* x_dev, int loss, double f_scale, double* f_true_dev, double* f_dev, double* Jc_dev,
                        double* Jp_dev, double* w_dev, void* stream);
int df3d_ba_robust_cost(const double* f_dev, size_t m, int loss, double f_scale, double* result_host, double* scratch_dev, void* stream);
int df3d_ba_trf_linearize_robust(const df3d_ba_problem* p, const double* x_dev, int loss, double f_scale, double* f_true_dev, double* f_dev,
                                 double* Jc_dev, double* Jp_dev, double* w_dev, double* g_dev, double* colsq_dev, double* scale_inv_dev,
                                 double* scale_dev, int first, double* scratch_dev, void* stream);
int df3d_ba_trf_trial_robust(const df3d_ba_problem* p, int loss, double f_scale, double p0, double p1, const double* s0_dev, const double* s1_dev,
                             const double* Js0_dev, const double* Js1_dev, const double* scale_dev, const double* x_dev, const double* g_h_dev,
                             double* step_h_dev, double* tmp_m_dev, double* step_dev, double* x_new_dev, double* f_new_dev, double* scratch_dev,
                             double* out_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a2  stacked-hourglass forward.   Replaces the network forward inside df2d's inference_folder
 *     (call site reference df3d/core.py:177-185; 2 stacks / 19 maps / 64x128 heat-maps:
 *     reference df3d/config.py:18,33,36).
 *
 * The engine owns the layer plan (which convolution follows which); the caller owns all memory:
 *   1. df3d_hg_create(dtype, num_stacks, &h)
 *   2. for i in [0, df3d_hg_num_params(h)): df3d_hg_param_desc(h, i, &d) names one packed tensor
 *      (e.g. "layer1.0.conv1") with its shape; the caller fills a float32 host blob of
 *      df3d_hg_blob_floats(h) floats at d.offset and uploads it:  df3d_hg_set_weights(h, blob_dev, ...).
 *      Packed layout per convolution: weight [taps][cout_pad][cin_pad] (k contiguous), bias[cout_pad],
 *      and for pre-activated convs in_scale[cin_pad], in_shift[cin_pad] (eval-mode BN as y = x*s + t).
 *      The stem ("conv1", taps = 49) is packed [148][64]: row k = ky*21 + kx*3 + c, 64 outputs contiguous (its slot
 *      is 184*64 floats: bf16 engines re-lay the low-precision copy as a [64][184] tile; leave the tail zero).
 *      BatchNorms that FOLLOW a convolution are folded into its weight/bias by the caller (the Python packer
 *      deepfly3d_amd/hourglass.py does this in float64).
 *   3. df3d_hg_forward(h, images_dev, n, heatmaps_dev, workspace_dev, workspace_bytes, stream)
 *      images_dev   [n, 256, 512, 3] float32 NHWC      (any H, W multiple of 64 via df3d_hg_set_input)
 *      heatmaps_dev [n, 19, H/4, W/4] float32 NCHW
 *      workspace    >= df3d_hg_workspace_bytes(h, n)
 * ---------------------------------------------------------------------------------------------- */
typedef struct df3d_hg df3d_hg;

typedef struct df3d_hg_param {
    char name[64];   /* e.g. "hg.0.hg.3.0.0.conv2"                                    */
    int kind;        /* 0 weight, 1 bias, 2 in_scale, 3 in_shift                       */
    int taps;        /* 1, 9 or 49                                                     */
    int cin, cout;   /* logical sizes                                                  */
    int cin_pad, cout_pad;
    size_t offset;   /* in floats, into the blob                                       */
    size_t count;    /* in floats                                                      */
    int kperm;       /* 1: weight K (cin) order is permuted inside every 32-channel group: packed position
                        8*(2q + h) + e holds channel 16q + 8*(e>>2) + 4h + (e&3)  (q, h in {0,1}, e in 0..7);
                        used by the bf16 fused bottleneck, whose conv3 consumes MFMA accumulators directly */
    int reserved;
} df3d_hg_param;

int df3d_hg_create(int dtype, int num_stacks, df3d_hg** out);
void df3d_hg_destroy(df3d_hg* h);
int df3d_hg_set_input(df3d_hg* h, int height, int width);
int df3d_hg_num_params(const df3d_hg* h);
int df3d_hg_param_desc(const df3d_hg* h, int i, df3d_hg_param* out);
size_t df3d_hg_blob_floats(const df3d_hg* h);
/* Engine-private device copies of the weights, made by df3d_hg_set_weights in a caller-owned buffer of
 * df3d_hg_lowp_bytes(h) bytes (256-byte aligned; NULL is accepted when that size is 0): the bf16 copy of the blob (bf16
 * engines) and, for both dtypes, the "weight streams" of the 256 -> 128 -> 128 -> 256 bottlenecks -- their weights repacked
 * as the sequence of 8 KB LDS images the kernel pulls through its LDS-DMA ring (option "ring", default 1); bf16 engines also
 * keep the heads' fc / fc_ / score_ weights in that form and layer1's whole weight set as one LDS image (option "l1").
 * DF3D_DTYPE_F32S: a float32-sized copy of the blob with every 16-float K step of every weight row stored as its IEEE-half hi / lo
 * parts in MFMA operand order (and the stem's weights as two half-precision tiles), followed by the streams packed from that copy;
 * lowp_dev must not be NULL. */
size_t df3d_hg_lowp_bytes(const df3d_hg* h);
int df3d_hg_set_weights(df3d_hg* h, const float* blob_dev, void* lowp_dev, void* stream);
/* knobs: "fuse" = 1 (default) | 0: run 256->128->128->256 bottlenecks as one fused kernel -- must be set before
 * the weights (it changes the manifest);  "fuse_upadd" = 1 (default) | 0: the hourglass'
 * nearest-upsample + add is folded into the input load of the bottleneck that consumes the sum (same results bit
 * for bit; set before the weights);  "row_bytes" = 0 (auto) | 64 | 128 bytes staged per operand row per K-step;
 * "ring" = 1 (default) | 0: weights through LDS-DMA stage rings (see df3d_hg_lowp_bytes) or register-staged;  "l1" = 1
 * (default) | 0: bf16 layer1 as the LDS-resident-weights kernel that writes only the pooled tensor -- both set before the
 * weights, both bit-identical to their 0 form;  "split1" = 1 (default) | 0 (fp32): conv1 of every bottleneck (layer1 / layer2 included) once per
 * pixel in a kernel of its own, the rest in tail kernels (17 MB more workspace per view: query df3d_hg_workspace_bytes);  "w2d" = 1 (default) | 0 (16-bit): the 3x3's weights of the ring bottlenecks as per-wave MFMA
 * fragments loaded straight from global memory (288 KB more stream space per bottleneck) -- both before the weights, both
 * bit-identical to their 0 form;  "chain_views" = 0 (default) | n: chains of full-resolution steps in chunks of n views;
 * "no_reuse" = 0 (default) | 1: the alias-free workspace plan (no tensor is ever given memory another tensor has released: ~5x the workspace) --
 * the reference form the aliasing tests compare the default plan with, bit for bit; before the weights;
 * "wino" = 1 (default) | 0 (exact fp32 with "split1"): the 3x3 of the 256->128->128->256 identity blocks (and layer2's) as Winograd F(2x4, 3x3) -- 24 instead
 * of 72 multiplies per 2x4 output patch and (cin, cout) pair -- and layer1's as F(2x2, 3x3), 1 MB more stream space per block; the SAME float32 tolerance against
 * the reference arithmetic, but NOT bit-identical
 * to the direct form ("wino" = 0: the bit-identity reference of the other options); before the weights;
 * "c1res" = 1 (default) | 0 (with "wino"): conv1 of the plain identity blocks with its 128 KB of weights resident in LDS (128 KB more stream space per block,
 * allocated with "wino") instead of streamed through the LDS ring -- bit-identical either way; may be set between forwards */
int df3d_hg_set_option(df3d_hg* h, const char* key, int value);
size_t df3d_hg_workspace_bytes(const df3d_hg* h, int n);
int df3d_hg_forward(df3d_hg* h, const float* images_dev, int n, float* heatmaps_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);
/* The same forward pass fed with the camera frames themselves: frames_dev [n][frame_h][frame_w][frame_c] uint8 (frame_c = 1 or
 * 3), flip_dev [n] uint8 or NULL (non-zero: mirror the frame left-right).  The stem samples its input patches from the frames
 * with the arithmetic of df3d_preprocess_u8 (`resize` rule to the engine's input size, (v/255 - mean) / std), so the result is bit
 * for bit df3d_hg_forward(df3d_preprocess_u8(frames)) without the float image in between (the call df2d's dataset +
 * network make per batch, behind reference df3d/core.py:177-185). */
int df3d_hg_forward_u8(df3d_hg* h, const unsigned char* frames_dev, const unsigned char* flip_dev, int n, int frame_h, int frame_w,
                       int frame_c, const float* mean3_host, const float* std3_host, int resize, float* heatmaps_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);
/* algorithmic work of one forward over n views: FLOPs and activation bytes (fusion model M1 of
 * SURVEY.md 8d evaluated on this engine's own plan) */
int df3d_hg_work(const df3d_hg* h, int n, double* flops, double* bytes);
/* per-kernel timing with HIP events recorded on the launch stream around every launch (small overhead: enable it
 * for a measurement pass only).  Launches are grouped by kernel instantiation, named as rocprofv3 prints them
 * (e.g. "bottleneck_kernel<float, 256, 128, false>").  df3d_hg_profile(h, 1) clears previous samples;
 * df3d_hg_profile_count() = number of distinct kernels seen; df3d_hg_profile_read() waits for the events and
 * returns name, summed duration (ms), algorithmic FLOPs, two byte figures and the launch count of kernel `index`:
 * bytes = the minimum the launches can move (their inputs read once, their outputs written once, fused intermediates on
 * chip), bytes_m1 = what the fusion model M1 of SURVEY.md 8(d) charges for the same plan steps (every convolution's input
 * and output once, pooling and upsample passes) -- the convention df3d_hg_work() sums.  (Round 3 added bytes_m1.) */
int df3d_hg_profile(df3d_hg* h, int enable);
int df3d_hg_profile_count(const df3d_hg* h);
int df3d_hg_profile_read(df3d_hg* h, int index, char* name_buf, int buflen, double* ms, double* flops, double* bytes, double* bytes_m1,
                         int* launches);
/* (round 6) FLOPs the launches of kernel `index` EXECUTED on the matrix pipe, summed like df3d_hg_profile_read's `flops`.  Equal to `flops` (the
 * direct-convolution count of the plan steps, the reference's arithmetic) for every kernel except the Winograd tail of option "wino", which does a
 * 3x3 with 16/36 of the direct form's multiplies: a roofline fraction is executed FLOPs over peak, never direct-equivalent FLOPs over peak. */
int df3d_hg_profile_executed_flops(df3d_hg* h, int index, double* flops_executed);
/* debugging / layer-wise parity: number of plan steps, and run only steps [0, upto) then copy the
 * tensor produced by step upto-1 (NHWC, engine dtype widened to float32) into out_dev */
int df3d_hg_num_steps(const df3d_hg* h);
/* model-M1 bytes of plan step `step` over n views (the steps' values sum to df3d_hg_work()'s bytes) */
double df3d_hg_step_m1_bytes(const df3d_hg* h, int step, int n);
int df3d_hg_step_desc(const df3d_hg* h, int step, char* name_buf, int buflen, int* n_h_w_c /*[3]: h, w, c*/);
/* the 2x2 max-pooled tensors plan step `step` writes beside its output: bit 0 the pooled output, bit 1 the pooled input (< 0: an error).
 * A step whose output IS the pooled tensor (layer1 when nothing else reads its full-resolution output) writes nothing beside it: 0 */
int df3d_hg_step_pooled(const df3d_hg* h, int step);
int df3d_hg_forward_upto(df3d_hg* h, const float* images_dev, int n, int upto, float* out_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * f4  frames of the pose videos (reference df3d/video.py:21-108, called from df3d/cli.py:308-321).  One launch draws one frame:
 *     every output pixel tests itself against the joints and bones of its camera (rule restated in oracle/render.py).
 * df3d_render_pose2d_grid: luma_dev [6, height, width] uint8 = the images of cameras (0, 1, 2 / 4, 5, 6) in that order;
 *     points_px_dev [6, num_joints, 2] float64 (row_px, col_px), a joint with a 0 coordinate is unseen; bones_host [num_bones, 2] and
 *     joint_rgb_host [num_joints, 3] (colour of a joint; a bone takes its first joint's) are HOST tables (<= 64 joints, <= 96 bones);
 *     out_rgb_dev [2 height, 3 width, 3] uint8: grey image, bone segments of thickness line_width, joint discs of `radius` on top.
 * df3d_render_pose3d_panels: points3d_dev [num_joints, 3] float64 (the pose Core.get_points3d returns for one image), three square
 *     panels [size, 3 size, 3] uint8, orthographic views from azimuth_deg3[k] / elevation_deg (matplotlib's view_init angles,
 *     reference df3d/plot_util.py:48-51), +-lim mapped onto the panel, black background.
 * df3d_resize_rgb: bilinear, pixel centres at half integers (cv2.INTER_LINEAR's geometry); pitches in pixels.
 * Rows go on the launch grid's y axis: height, size and out_h are at most 65535 (DF3D_EINVAL beyond, nothing launched).
 * All asynchronous on `stream`. */
int df3d_render_pose2d_grid(const unsigned char* luma_dev, int height, int width, const double* points_px_dev, int num_joints,
                            const int* bones_host, int num_bones, const unsigned char* joint_rgb_host, double radius, double line_width,
                            unsigned char* out_rgb_dev, void* stream);
int df3d_render_pose3d_panels(const double* points3d_dev, int num_joints, const int* bones_host, int num_bones,
                              const unsigned char* joint_rgb_host, const double* azimuth_deg3, double elevation_deg, double lim, int size,
                              double line_width, unsigned char* out_rgb_dev, void* stream);
int df3d_resize_rgb(const unsigned char* in_dev, int in_h, int in_w, int in_pitch_px, unsigned char* out_dev, int out_h, int out_w,
                    int out_pitch_px, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Heat-map overlays: the network's heat-maps drawn on the camera images, one launch per frame.
 * df3d_render_heatmap: luma_dev [num_slots, height, width] uint8 and heatmaps_dev [num_slots, num_planes, hm_height, hm_width] float32, one
 *     view per slot (1..8); num_selected_host [num_slots] (0..32 each), planes_host and rgb_host hold the selected plane indices and their
 *     RGB colours slot after slot ([sum n] and [sum n, 3]; may be null when nothing is selected), flip_host [num_slots] says whether the
 *     network saw the view mirrored: all HOST tables.  Output pixel (y, x) of a slot samples every selected plane bilinearly at
 *     (y hm_height / height, xs hm_width / width), xs = x or width - x when flipped (the arg-max convention: a plane's peak lands where
 *     its detection is drawn), a = clamp(gain * value, 0, 1), a non-finite tap reads as 0; the plane of largest a wins (ties: the
 *     earliest) and the pixel is floor((1 - a) grey + a colour + 0.5).  out_rgb_dev [ceil(num_slots / cols) height, cols width, 3] uint8,
 *     slot s at grid cell (s / cols, s % cols); cells past the last slot are not written.  float64 arithmetic without multiply-add
 *     fusion, restated in tests/heatmap_overlay_oracle.py.  Arguments are validated before the launch (DF3D_EINVAL: slots, columns,
 *     sizes, a gain that is negative or not finite, a plane index outside [0, num_planes), a null pointer).  Asynchronous on `stream`. */
int df3d_render_heatmap(const unsigned char* luma_dev, int height, int width, const float* heatmaps_dev, int num_planes, int hm_height,
                        int hm_width, int num_slots, int cols, const int* num_selected_host, const int* planes_host,
                        const unsigned char* rgb_host, const unsigned char* flip_host, double gain, unsigned char* out_rgb_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DF3D_HIP_H */
