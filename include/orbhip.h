/*
 * orbhip.h -- C ABI of liborbhip.so: ORB-SLAM3's per-frame feature front end on MI355X (gfx950).
 *
 * Drop-in boundary.  The reference has no plugin/FFI layer: the boundary is the two C++
 * classes ORB_SLAM3::ORBextractor (include/ORBextractor.h:43-109) and ORB_SLAM3::ORBmatcher
 * (include/ORBmatcher.h:35-108).  3_orb_slam3_selfnote_amd/csrc/adapter/ re-declares those classes with identical
 * signatures and forwards to the entry points below; INTEGRATION.md shows the two-line CMake change.
 *
 * Plain pointers and sizes only.  "host" entry points take host memory and synchronise before returning;
 * "_device" entry points take device memory, are asynchronous on `stream` (a hipStream_t passed as void*,
 * used verbatim: NULL = the device's default stream) and never touch the host.
 *
 * Return convention: >= 0 success (function specific), < 0 error:
 *   ORBX_E_EMPTY (-1)  empty image            (ORBextractor.cc:1075-1076 returns -1)
 *   ORBX_E_ARG   (-2)  bad argument / unsupported geometry
 *   ORBX_E_HIP   (-3)  HIP runtime error, see orbx_last_error()
 *   ORBX_E_CAP   (-4)  caller capacity too small (n_out holds the required count)
 */
#ifndef ORBHIP_H
#define ORBHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_E_EMPTY (-1)
#define ORBX_E_ARG (-2)
#define ORBX_E_HIP (-3)
#define ORBX_E_CAP (-4)
#define ORBX_MAX_LEVELS 16

/* Same field order and size (28 B) as cv::KeyPoint, so a std::vector<cv::KeyPoint>::data() can be passed. */
typedef struct {
  float x, y;     /* pt */
  float size;     /* PATCH_SIZE * scale truncated to int (ORBextractor.cc:862, :871) */
  float angle;    /* degrees [0,360), IC_Angle (ORBextractor.cc:75-102) */
  float response; /* FAST score */
  int32_t octave;
  int32_t class_id; /* always -1 */
} orbx_keypoint_t;

typedef struct orbx_handle orbx_t;

/* ---- ORBextractor ------------------------------------------------------------------------------------------ */

/* ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
 * (ORBextractor.cc:408-468).  `device` = HIP device ordinal.  Returns NULL on failure. */
orbx_t *orbx_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device);
void orbx_destroy(orbx_t *h);
const char *orbx_last_error(const orbx_t *h);

/* Getters of ORBextractor.h:61-81.  Arrays must hold nlevels entries; any pointer may be NULL. */
int orbx_get_levels(const orbx_t *h);
float orbx_get_scale_factor(const orbx_t *h);
int orbx_get_scale_tables(const orbx_t *h, float *scaleFactors, float *invScaleFactors, float *levelSigma2,
                          float *invLevelSigma2);
int orbx_get_features_per_level(const orbx_t *h, int *nPerLevel);

/* Size the device workspace for `max_batch` frames of rows x cols.  Called implicitly by the extract entry points
 * when the geometry changes.  Returns the per-frame keypoint capacity bound (sum over levels of the octree's
 * maximum output), which is what `cap` must be >= for orbx_extract* never to return ORBX_E_CAP.
 * Limits (ORBX_E_ARG with orbx_last_error otherwise): images up to 4096 x 4096, batches up to 65535 frames, and a
 * per-level feature quota (mnFeaturesPerLevel, ORBextractor.cc:432-443) of about 2200 -- DistributeOctTree's node list of a
 * level lives in the 160 KB of LDS; the reference's settings (1000-2000 features, the 5x initialisation extractor at 8
 * levels) stay below it. */
int orbx_configure(orbx_t *h, int rows, int cols, int max_batch);
int orbx_max_keypoints(const orbx_t *h);

/* int ORBextractor::operator()(InputArray image, InputArray mask, vector<KeyPoint>&, OutputArray descriptors,
 *                              vector<int>& vLappingArea)              (ORBextractor.cc:1071-1184)
 * image: host, CV_8UC1, rows x cols, `stride` bytes per row.  lap0/lap1 = vLappingArea[0..1].
 * Writes *n_out keypoints (28 B each) and *n_out x 32 descriptor bytes in the reference's output order and
 * returns monoIndex (ORBextractor.cc:1183).  `mask` is ignored by the reference (ORBextractor.h:56). */
int orbx_extract(orbx_t *h, const uint8_t *image, int rows, int cols, size_t stride, int lap0, int lap1,
                 orbx_keypoint_t *keypoints, uint8_t *descriptors, int cap, int *n_out);

/* Batched, device-resident form of the same call: frame f is at d_images + f*frame_stride.
 * d_keypoints: [nframes][cap] orbx_keypoint_t, d_descriptors: [nframes][cap][32], d_counts: [nframes][2] int32 =
 * {n, monoIndex}.  All device pointers; asynchronous on `stream`.  The level-0 image of each frame is read in
 * place, so d_images must stay valid until the stream has drained - and for as long as orbx_compute_stereo_matches or
 * orbx_download_level(level 0) may still be called for this batch (both order themselves behind the batch's last kernel
 * with an event, whatever stream it ran on).  cap must be >= orbx_configure()'s return value (ORBX_E_CAP otherwise: an
 * overflow could not be reported asynchronously, and d_counts is what the batched matcher takes as live counts). */
int orbx_extract_batch_device(orbx_t *h, const uint8_t *d_images, int rows, int cols, size_t stride,
                              size_t frame_stride, int nframes, int lap0, int lap1, orbx_keypoint_t *d_keypoints,
                              uint8_t *d_descriptors, int32_t *d_counts, int cap, void *stream);

/* std::vector<cv::Mat> ORBextractor::mvImagePyramid (ORBextractor.h:83) of the most recent call:
 * geometry, and a lazy download of one level of one frame of the last batch.  border = 0 copies the ROI;
 * border = 19 (EDGE_THRESHOLD) also synthesises the BORDER_REFLECT_101 frame of ORBextractor.cc:1203-1215. */
int orbx_level_info(const orbx_t *h, int level, int *rows, int *cols);
int orbx_download_level(orbx_t *h, int frame, int level, int border, uint8_t *dst, size_t dst_stride);
/* All levels of one frame at once, each with its `border`-pixel BORDER_REFLECT_101 frame, packed into dst: level l starts at
 * dst + offsets[l] with strides[l] bytes per row (offsets / strides: nlevels entries, written by the call).  One kernel, one
 * device-to-host copy, one synchronisation - what the extractor adapter uses to fill mvImagePyramid when a caller still reads
 * it on the host (the reference's own Frame::ComputeStereoMatches).  dst == NULL: only offsets / strides and the size.
 * Returns the number of bytes (ORBX_E_CAP if dst_bytes is smaller). */
int orbx_download_pyramid(orbx_t *h, int frame, int border, uint8_t *dst, size_t dst_bytes, size_t *offsets, size_t *strides);

/* Stage taps for parity tests (same data the pipeline consumes; host pointers, synchronous).  Valid after an
 * extract call, for frame index `frame` of that call. */
int orbx_download_blurred_level(orbx_t *h, int frame, int level, uint8_t *dst, size_t dst_stride);
/* FAST candidates of one level, i.e. vToDistributeKeys of ORBextractor.cc:776-850 in the reference's order:
 * xyr[3*i..] = (x, y, response) relative to (minBorderX, minBorderY).  Returns the count. */
int orbx_download_candidates(orbx_t *h, int frame, int level, float *xyr, int cap);
/* DistributeOctTree output of one level (ORBextractor.cc:859-860), list order, same coordinates. */
int orbx_download_level_keypoints(orbx_t *h, int frame, int level, float *xyr, int cap);

/* Host-side split of the last orbx_extract call, microseconds: us[0] copy of the image into pinned staging, us[1] submission of
 * the frame's sequence (one graph launch), us[2] wait for its completion, us[3] copy of the results into the caller's arrays.
 * Returns 4.  Diagnostic (tools/latency_breakdown.py); no counterpart in the reference. */
int orbx_get_host_us(const orbx_t *h, float *us, int cap);

/* Per-stage GPU time, measured with HIP events recorded on the stream the kernels were launched on.
 * orbx_set_profiling(h, 1) starts (or restarts) a recording; every extract call after it records one event set into a ring of
 * 32, and orbx_get_stage_ms returns the per-stage AVERAGE over the calls recorded since then (the 32 most recent): one
 * call = "the last call", a whole timed region = its average.  Stages: 0 pyramid, 1 fast, 2 octree, 3 blur,
 * 4 orient+describe.  Returns the number of stages written (ms). */
void orbx_set_profiling(orbx_t *h, int enable);
int orbx_get_stage_ms(orbx_t *h, float *ms, int cap);

/* Device replica of the libm cosf/sinf the reference calls at ORBextractor.cc:111, exposed for the exhaustive
 * host-side check in tests (host evaluation of the same source the kernel compiles). */
float orbx_ref_cosf(float x);
float orbx_ref_sinf(float x);
/* Likewise the device replicas of glibc's atanf / atan2f (fdlibm single precision) used by the on-device
 * KannalaBrandt8::project (KannalaBrandt8.cpp:31-32), csrc/orb_atan2f.h. */
float orbx_ref_atanf(float x);
float orbx_ref_atan2f(float y, float x);
/* ... and of glibc's logf (ARM optimized-routines, glibc >= 2.28) that MapPoint::PredictScale calls (MapPoint.cc:587-602),
 * csrc/orb_logf.h: the level prediction of orbm_search_local_points on the device. */
float orbx_ref_logf(float x);
/* The same replica evaluated by the DEVICE: d_y[i] = logf(d_x[i]) for i < n, device pointers, asynchronous on `stream`
 * (tests/test_gpu_local_points.py compares it with orbx_ref_logf).  Returns 0, ORBX_E_ARG or ORBX_E_HIP. */
int orbx_logf_device(const float *d_x, int n, float *d_y, void *stream);
/* ... and of glibc's tanf (fdlibm's single-precision kernel behind the double reduction of sinf / cosf, glibc 2.28 - 2.40) that
 * KannalaBrandt8::unproject calls (KannalaBrandt8.cpp:135), csrc/orb_tanf.h, for every float (the integer reduction from |x| = 120 on); orbx_tanf_device is the
 * device's evaluation, as orbx_logf_device. */
float orbx_ref_tanf(float x);
int orbx_tanf_device(const float *d_x, int n, float *d_y, void *stream);
/* The other scalar functions the kernels restate, evaluated by the DEVICE with the contract of orbx_logf_device: cosf / sinf
 * (csrc/orb_sincos.h, |x| < 120), atanf / atan2f (csrc/orb_atan2f.h; d_out[i] = atan2f(d_yin[i], d_xin[i])) and the kernels' cv::fastAtan2
 * (fast_atan2_deg of csrc/orb_kernels.h, degrees in [0, 360]; it has no host build).  Each launches one elementwise kernel that calls the
 * inline function the production kernels call; tests/test_gpu_libm_device.py compares the results with orbx_ref_*, with the host
 * glibc and with the oracle's fastAtan2 on the input sets of tests/libm_device_cases.py. */
int orbx_cosf_device(const float *d_x, int n, float *d_y, void *stream);
int orbx_sinf_device(const float *d_x, int n, float *d_y, void *stream);
int orbx_atanf_device(const float *d_x, int n, float *d_y, void *stream);
int orbx_atan2f_device(const float *d_yin, const float *d_xin, int n, float *d_out, void *stream);
int orbx_fast_atan2_device(const float *d_yin, const float *d_xin, int n, float *d_out, void *stream);

/* cv::cvtColor(im, gray, CV_RGB2GRAY | CV_BGR2GRAY | CV_RGBA2GRAY | CV_BGRA2GRAY) of Tracking::GrabImageMonocular / Stereo / RGBD
 * (Tracking.cc:1122-1135) for 8-bit input: channels = 3 or 4, rgb_order != 0 for RGB(A), 0 for BGR(A).
 * Fixed point as in OpenCV 3.x: (R*4899 + G*9617 + B*1868 + 8192) >> 14.  *_device: device pointers, asynchronous on stream. */
int orbx_cvt_color_gray_device(const uint8_t *d_src, int rows, int cols, size_t src_stride, int channels, int rgb_order, uint8_t *d_dst,
                               size_t dst_stride, void *stream);
int orbx_cvt_color_gray(orbx_t *h, const uint8_t *src, int rows, int cols, size_t src_stride, int channels, int rgb_order, uint8_t *dst,
                        size_t dst_stride);

/* cv::CLAHE::apply for CV_8UC1 as the TUM-VI examples call it on every image before Track* (Examples/Monocular/mono_tum_vi.cc:101-109,
 * Monocular-Inertial/mono_inertial_tum_vi.cc:128, Stereo-Inertial/stereo_inertial_tum_vi.cc:132: createCLAHE(3.0, Size(8, 8))).
 * OpenCV 3.4/4.x algorithm: per-tile clipped histogram (excess spread as batch + every residualStep-th bin), cumulative LUT,
 * float bilinear blend of the four neighbouring tiles' LUTs; sizes that are not a multiple of the tile grid are extended with
 * BORDER_REFLECT_101 for the histograms.  tiles_x * tiles_y <= 256.  src == dst (in place, as the examples do) is allowed.
 * *_device: device pointers, asynchronous on stream; d_lut is tiles_x*tiles_y*256 bytes of device scratch. */
int orbx_clahe_device(const uint8_t *d_src, int rows, int cols, size_t src_stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *d_lut,
                      uint8_t *d_dst, size_t dst_stride, void *stream);
int orbx_clahe(orbx_t *h, const uint8_t *src, int rows, int cols, size_t src_stride, double clip_limit, int tiles_x, int tiles_y, uint8_t *dst,
               size_t dst_stride);

/* cv::remap(src, dst, M1, M2, cv::INTER_LINEAR) with CV_32FC1 maps and the default BORDER_CONSTANT(0): the stereo rectification of
 * Examples/Stereo/stereo_euroc.cc:166-167 (maps from initUndistortRectifyMap, :113-114, computed once by the caller).
 * dst is rows x cols like the maps; coordinates are quantised to 1/32 px and blended with OpenCV's 15-bit fixed-point weights.
 * orbx_remap_linear keeps the uploaded maps: pass mapx = mapy = NULL on later calls to reuse them. */
int orbx_remap_linear_device(const uint8_t *d_src, int src_rows, int src_cols, size_t src_stride, const float *d_mapx, const float *d_mapy,
                             size_t map_stride_elems, int rows, int cols, uint8_t *d_dst, size_t dst_stride, void *stream);
int orbx_remap_linear(orbx_t *h, const uint8_t *src, int src_rows, int src_cols, size_t src_stride, const float *mapx, const float *mapy, int rows,
                      int cols, uint8_t *dst, size_t dst_stride);

/* orbx_clahe_device / orbx_remap_linear_device for `nframes` frames resident in HBM, one call per batch.  No handle: device
 * pointers, asynchronous on `stream`, no host synchronisation, copy or allocation.  Frame f is at d_src + f * src_frame_stride, its
 * result goes to d_dst + f * dst_frame_stride; per frame the bytes are those of the per-image call.  Bytes of d_dst outside the
 * rows x cols of each frame (row padding, padding between frames) are not written.  nframes == 0 returns 0 and launches nothing.
 *
 * orbx_clahe_batch_device: d_lut is nframes * tiles_x * tiles_y * 256 bytes of device scratch.  In place (d_dst == d_src with equal
 * row and frame strides, as the examples do) is allowed.  Two kernels: the tables of all tiles of all frames (grid tile x frame,
 * one sub-histogram per wavefront), then the blend in bands of ORBX_CLAHE_BAND_ROWS image rows (grid band x frame) that stage only
 * the table rows a band reads.  ORBX_E_ARG: what orbx_clahe_device refuses, nframes < 0, for nframes > 1 a frame stride smaller than
 * (rows - 1) * stride + cols, and source and destination ranges that intersect in any way other than the in-place form.
 *
 * orbx_remap_linear_batch_device: one map pair serves all frames (it is fixed per camera).  One kernel: a thread decodes the map
 * entry of its output pixel once and applies it to ORBX_REMAP_FRAME_CHUNK frames.  ORBX_E_ARG: what orbx_remap_linear_device
 * refuses, nframes < 0, for nframes > 1 a frame stride smaller than (rows - 1) * stride + cols of its side, and a destination range
 * that intersects the source range (cv::remap goes through a temporary when called in place; this call has none).
 * Both return 0, ORBX_E_ARG or ORBX_E_HIP. */
#define ORBX_CLAHE_BAND_ROWS 32
#define ORBX_REMAP_FRAME_CHUNK 16
int orbx_clahe_batch_device(int nframes, const uint8_t *d_src, int rows, int cols, size_t src_stride, size_t src_frame_stride, double clip_limit,
                            int tiles_x, int tiles_y, uint8_t *d_lut, uint8_t *d_dst, size_t dst_stride, size_t dst_frame_stride, void *stream);
int orbx_remap_linear_batch_device(int nframes, const uint8_t *d_src, int src_rows, int src_cols, size_t src_stride, size_t src_frame_stride,
                                   const float *d_mapx, const float *d_mapy, size_t map_stride_elems, int rows, int cols, uint8_t *d_dst,
                                   size_t dst_stride, size_t dst_frame_stride, void *stream);
/* Host arithmetic of the launch code above, exposed for tests/test_preops_batch_abi.py: the table rows (tile rows) the blend reads for
 * the image rows y0 .. y1 of a rows-high image with tiles_y tile rows: *first, *count.  ORBX_E_ARG unless 0 <= y0 <= y1 < rows,
 * 0 < tiles_y <= rows and both pointers are given.  Returns 0. */
int orbx_clahe_band_lut_rows(int rows, int tiles_y, int y0, int y1, int *first, int *count);

/* void Frame::ComputeStereoMatches()  (Frame.cc:901-1079), rectified stereo - the consumer of mvImagePyramid.
 * left / right: the two extractors (mpORBextractorLeft / Right) AFTER orbx_extract / orbx_extract_batch_device of the
 * two images: their pyramids are still on the device (frame_l / frame_r = index in their last batch), so no image
 * crosses PCIe again.  keysL / descL, keysR / descR = mvKeys / mDescriptors, mvKeysRight / mDescriptorsRight (host);
 * mb, mbf = Frame::mb, mbf.  uRight[nL], depth[nL] (out) = mvuRight, mvDepth.  The descriptor search, the 11x11 SAD
 * refinement and the parabola fit run on the device (one wavefront per left keypoint); the median filter over the
 * accepted matches (:1060-1073) needs a sort and runs on the host.  Returns 0. */
int orbx_compute_stereo_matches(orbx_t *left, int frame_l, orbx_t *right, int frame_r, int nL, const orbx_keypoint_t *keysL,
                                const uint8_t *descL, int nR, const orbx_keypoint_t *keysR, const uint8_t *descR, float mb,
                                float mbf, float *uRight, float *depth);

/* The same member (Frame.cc:901-1079) for `nframes` frame pairs resident in HBM, asynchronous on `stream`: no host
 * synchronisation, no host copy, no host arithmetic.  left / right: the two extractors after orbx_extract_batch_device of
 * nframes (or more) left and right images with lapping area {0, 0} (Frame.cc:120-121); frame f of one is paired with frame f of
 * the other.  d_keysL / d_descL / d_countsL and d_keysR / d_descR / d_countsR are exactly what those two calls wrote
 * ([nframes][cap], [nframes][cap][32], [nframes][2]); the pyramids are read from the handles' last batch, level 0 in place from
 * the caller's images (lifetime rule of orbx_extract_batch_device), ordered behind both extractions by their events.
 * d_uRight / d_depth [nframes][cap] = mvuRight / mvDepth: entries i < n_left(f) are written (-1 where the reference leaves -1),
 * entries beyond are left alone.  d_nstereo[f] (may be NULL) = number of entries >= 0 after the median filter.
 * Three kernels: the row table of :911-928 as 8-row bands on the device, the descriptor search over the band of each left
 * keypoint (:941-979) with the 11x11 SAD refinement and parabola fit (:982-1062), and the median filter (:1065-1078) as a rank
 * selection by two 256-bin histogram passes (no sort; no accepted match = nothing to do, as in the host form).  Same bits as
 * orbx_compute_stereo_matches per frame.  Scratch is grow-only device memory of `left` (growing it on a first, larger call is the
 * one step that blocks); calls on the same `left` handle share it, so issue them on one stream or order them yourself.
 * ORBX_E_ARG (with orbx_last_error(left)): NULL handle or required pointer, nframes outside the two handles' last batches, handles
 * that differ in device / image size / pyramid, mb <= 0, cap below orbx_max_keypoints, cap > 65535 (the 16-bit right index of
 * the search key, the host form's nR limit).  Returns 0. */
int orbx_compute_stereo_matches_batch_device(orbx_t *left, orbx_t *right, int nframes, const orbx_keypoint_t *d_keysL,
                                             const uint8_t *d_descL, const int32_t *d_countsL, const orbx_keypoint_t *d_keysR,
                                             const uint8_t *d_descR, const int32_t *d_countsR, int cap, float mb, float mbf,
                                             float *d_uRight, float *d_depth, int32_t *d_nstereo, void *stream);

/* void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)  (Frame.cc:1082-1103) for `nframes` RGB-D frames resident in HBM,
 * with the imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) of Tracking::GrabImageRGBD (Tracking.cc:1075-1076) evaluated only
 * at the keypoints.  No handle: device pointers, asynchronous on `stream`, no host synchronisation, copy or allocation.
 * d_keys / d_keys_un [nframes][cap] = mvKeys / mvKeysUn as orbx_extract_batch_device and orbm_undistort_keypoints_batch_device
 * wrote them; N of frame f = d_counts[f * count_stride].  Depth image of frame f at d_depth_image + f * frame_stride, rows x cols,
 * row_stride bytes per row; depth_type 0 = 16-bit unsigned (the TUM PNGs), 1 = float.  depth_factor = mDepthMapFactor as
 * Tracking.cc:751-755 leaves it (already the reciprocal; 1 for a float image the reference does not convert, :1075: the
 * product with 1.0f is exact).  mbf = Frame::mbf.
 * Per keypoint i < N: d = (float)raw * depth_factor at the pixel ((int)kp.pt.y, (int)kp.pt.x) of the DISTORTED keypoint, both
 * truncated as at<float>(v, u) converts its float arguments; d > 0: d_depth = d, d_uRight = kpU.pt.x - mbf / d; otherwise both
 * -1 (so NaN gives -1, +inf gives depth inf and uRight = kpU.pt.x).  Entries beyond N are left alone.  d_nstereo[f] (may be
 * NULL) = number of entries with depth > 0.  One deviation: a pixel outside rows x cols, undefined behaviour in the reference,
 * gives -1 here and is never read.
 * ORBX_E_ARG: a NULL required pointer, nframes < 0, cap <= 0, count_stride <= 0, rows / cols <= 0, depth_type not 0 / 1, a
 * row_stride smaller than a row or not a multiple of the element size, a frame_stride that is not such a multiple or (for
 * nframes > 1) smaller than an image.  Returns 0, ORBX_E_ARG or ORBX_E_HIP. */
int orbx_stereo_from_rgbd_batch_device(int nframes, const orbx_keypoint_t *d_keys, const orbx_keypoint_t *d_keys_un, const int32_t *d_counts,
                                       int count_stride, int cap, const void *d_depth_image, int depth_type, int rows, int cols, size_t row_stride,
                                       size_t frame_stride, float depth_factor, float mbf, float *d_uRight, float *d_depth, int32_t *d_nstereo,
                                       void *stream);

/* The depth-ordered close-point rule of Tracking::UpdateLastFrame (Tracking.cc:2808-2860) and Tracking::CreateNewKeyFrame
 * (:3345-3416) for `nframes` frames, on d_depth [nframes][cap] = mvDepth from the call above or from
 * orbx_compute_stereo_matches_batch_device; same calling rules as above.  Per frame, with N = d_counts[f * count_stride]:
 * the keypoints i < N with z > 0 in the order of sort(vDepthIdx) (z ascending, then i), visited up to and including the first
 * position with z > th_depth (mThDepth) and position + 1 > max_point (100 in the reference) - nPoints grows on every iteration
 * of both loops (:2849-2853, :3405-3409), so the break does not depend on the map.  With c = #{0 < z <= th_depth} and
 * m = #{z > 0} that is nvisit = min(m, max(c, max_point) + 1); the one point beyond is the reference's behaviour.
 * d_order[f][0 .. nvisit) = the keypoint indices in visiting order (later entries are left alone), d_nvisit[f] = nvisit.
 * d_close[f][2] (may be NULL) = nTrackedClose, nNonTrackedClose of Tracking::NeedNewKeyFrame (:3190-3200: 0 < z < th_depth),
 * from d_tracked [nframes][cap] = mvpMapPoints[i] && !mvbOutlier[i] (NULL: every point is untracked).
 * d_x3Dc [nframes][cap][3] (may be NULL; needs d_keys_un = mvKeysUn): Frame::UnprojectStereo (Frame.cc:1105-1116) in camera
 * coordinates for every i < N with z > 0, x = (u - cx) * z * invfx with invfx = 1.0f / fx (Frame.cc:275-276), y likewise; other
 * entries are left alone.  d_pose [nframes][12] = [mRwc | mOw] row-major 3x4 and d_x3Dw [nframes][cap][3] (both or neither;
 * need d_x3Dc): mRwc * x3Dc + mOw.
 * One workgroup per frame, the keys (bits(z) << 32 | i: positive floats order as their bit patterns) sorted in LDS, which holds
 * ORBX_CLOSE_MAX_KEYPOINTS of them.  ORBX_E_ARG: a NULL required pointer (d_depth, d_counts, d_order, d_nvisit), nframes < 0,
 * cap <= 0 or above ORBX_CLOSE_MAX_KEYPOINTS, count_stride <= 0, an incomplete unprojection set.  Returns 0, ORBX_E_ARG or
 * ORBX_E_HIP. */
#define ORBX_CLOSE_MAX_KEYPOINTS 4096 /* per frame: 32 KB of 8-byte keys; extractors of up to ~4000 features stay below it */
int orbx_close_points_batch_device(int nframes, const float *d_depth, const int32_t *d_counts, int count_stride, int cap, float th_depth, int max_point,
                                   int32_t *d_order, int32_t *d_nvisit, const uint8_t *d_tracked, int32_t *d_close, const orbx_keypoint_t *d_keys_un,
                                   float fx, float fy, float cx, float cy, float *d_x3Dc, const float *d_pose, float *d_x3Dw, void *stream);

/* ---- ORBmatcher -------------------------------------------------------------------------------------------- */

#define ORBM_TH_HIGH 100 /* ORBmatcher.cc:36 */
#define ORBM_TH_LOW 50   /* ORBmatcher.cc:37 */
#define ORBM_HISTO_LENGTH 30
#define ORBM_GRID_COLS 64 /* Frame.h:38 */
#define ORBM_GRID_ROWS 48 /* Frame.h:39 */
#define ORBM_MAX_KEYPOINTS 15360 /* per frame, projection search: its claim state lives in one CU's LDS */
/* Fisheye-stereo searches (orbm_search_by_projection_fisheye, ..._last_frame_fisheye) keep a partner list in LDS as well and
 * take up to about 13 000 keypoints (left + right); beyond that they return ORBX_E_ARG.  The resident forms
 * (orbm_rig_concat_batch_device, orbm_search_by_projection_last_frame_fisheye_batch_device) refuse a frame stride above
 * the count at which that list still fits: */
#define ORBM_FISHEYE_MAX_KEYPOINTS 12960

typedef struct orbm_handle orbm_t;
orbm_t *orbm_create(int device);
void orbm_destroy(orbm_t *m);
const char *orbm_last_error(const orbm_t *m);

/* static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&) (ORBmatcher.cc:2463-2483), host. */
int orbm_descriptor_distance(const uint8_t *a, const uint8_t *b);

/* The slice of Frame a projection search reads (mono / rectified stereo, Nleft == -1):
 * mvKeysUn (Frame.h: vector<cv::KeyPoint>, passed as its data()), mDescriptors, mvuRight, the grid bounds
 * mnMinX..mnMaxY (Frame.cc:872-899).  The 64x48 grid of Frame.cc:434-465 is not materialised: a candidate's
 * cell (PosInGrid, Frame.cc:815-825) is recomputed from its coordinates and the walk order of
 * GetFeaturesInArea (Frame.cc:781-809: ix outer, iy inner, insertion order) is carried as a sort key. */
typedef struct {
  int32_t n;
  const orbx_keypoint_t *keys_un;
  const uint8_t *descriptors; /* n x 32 */
  const float *u_right;       /* mvuRight, or NULL (all negative) */
  float min_x, max_x, min_y, max_y;
} orbm_frame_t;

/* One query = one map point already projected by the caller.
 * flags bit0: take part (mbTrackInView && !isBad ...), bit1: the map point has Observations()>0 (a keypoint it
 * claims is skipped by later queries, ORBmatcher.cc:89-91, :2135-2137). */
typedef struct {
  int32_t nq;
  const uint8_t *descriptors; /* nq x 32, MapPoint::GetDescriptor() */
  const float *u, *v;         /* projection (mTrackProjX/Y or camera->project) */
  const float *radius;        /* window half-size passed to GetFeaturesInArea */
  const int32_t *min_level, *max_level; /* GetFeaturesInArea level window, -1 = open */
  const float *u_r;           /* projected right coordinate for the rectified-stereo check, or NULL */
  const uint8_t *flags;       /* or NULL = all 0x3 */
} orbm_queries_t;

/* Projection search core shared by the five ORBmatcher::SearchByProjection overloads.
 * use_second != 0: best/second-best with the same-level ratio test of ORBmatcher.cc:104-129 (M2);
 * use_second == 0: strict-less argmin with threshold th_dist (M3 :2152-2162, M4 :2362-2371, M5 :586-600).
 * th_dist in [0, 255] (ORBX_E_ARG otherwise: at 256 the reference would accept a query that has no candidate at all).
 * slot[n] (in/out): query id holding keypoint i, -1 = free (F.mvpMapPoints); slot_obs[n] (in/out): 1 if that
 * holder has Observations()>0.  match_of_query[nq] (out, may be NULL); best_dist[nq] (out, may be NULL) = distance
 * of the best unclaimed candidate when it is <= th_dist, else 256.
 * Queries are resolved in index order with the reference's sequential claim semantics.  Returns nmatches. */
int orbm_search_by_projection(orbm_t *m, const orbm_frame_t *frame, const orbm_queries_t *q, float nnratio,
                              int th_dist, int use_second, int32_t *slot, uint8_t *slot_obs,
                              int32_t *match_of_query, int32_t *best_dist);

/* Batched device form: `npairs` independent (frame, query-set) problems.  Every pointer inside the two structs,
 * and slot/slot_obs/match_of_query/best_dist, is a device pointer to the data of problem 0; problem p is at
 * element offset p*frame_stride (keypoint-indexed arrays) resp. p*query_stride (query-indexed arrays).
 * d_frame_n[p] / d_query_n[p] give the live counts (device int32, e.g. orbx d_counts with stride 2).
 * A device count outside [0, stride] is taken into that range, here and in every batched form below.
 * d_nmatches[p] receives the match count.  Asynchronous on stream. */
int orbm_search_by_projection_batch_device(orbm_t *m, const orbm_frame_t *frame0, int frame_stride,
                                           const int32_t *d_frame_n, int frame_n_stride, const orbm_queries_t *q0,
                                           int query_stride, const int32_t *d_query_n, int query_n_stride,
                                           int npairs, float nnratio, int th_dist, int use_second, int32_t *d_slot,
                                           uint8_t *d_slot_obs, int32_t *d_match_of_query, int32_t *d_best_dist,
                                           int32_t *d_nmatches, void *stream);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
 * (ORBmatcher.cc:2027-2289, Nleft == -1 path), flattened.  Host pointers.
 * Last-frame side, i in [0, nLast): has_mp[i] = LastFrame.mvpMapPoints[i] && !LastFrame.mvbOutlier[i];
 * Xw[3i..] = pMP->GetWorldPos(); mpdesc[32i..] = pMP->GetDescriptor(); last_keys[i] = LastFrame.mvKeys[i]
 * (octave) / mvKeysUn[i] (angle); obs[i] = pMP->Observations()>0 (NULL = all 1).
 * Tcw / Tlw = CurrentFrame.mTcw / LastFrame.mTcw, row-major 4x4.  cam_type/cam_params: CurrentFrame.mpCamera
 * (see orbm_project).  mb, mbf: CurrentFrame.mb / mbf.  scale_factors = CurrentFrame.mvScaleFactors.
 * One upload, then projection (:2072-2097), window selection (:2105-2118), the Hamming search with its sequential claims and
 * the rotation-histogram pruning (:2177-2185, :2263-2286) all run on the device (see the batched form below), one download.
 * slot / slot_obs as in orbm_search_by_projection.  Returns nmatches. */
int orbm_search_by_projection_last_frame(orbm_t *m, const orbm_frame_t *cur, const float *scale_factors, int nlevels,
                                         int nLast, const uint8_t *has_mp, const float *Xw, const uint8_t *mpdesc,
                                         const orbx_keypoint_t *last_keys, const uint8_t *obs, const float *Tcw,
                                         const float *Tlw, int cam_type, const float *cam_params, float mb, float mbf,
                                         float th, int bMono, int checkOri, int32_t *slot, uint8_t *slot_obs);

/* Batched device form of the same member: `npairs` independent (current frame, last frame) problems, everything resident in
 * HBM, asynchronous on `stream`, nothing touches the host.  Projection (:2038-2118, Pinhole or KannalaBrandt8 with bit-exact
 * replicas of the libm calls), Hamming search with sequential claims (:2120-2162) and rotation pruning (:2177-2185, :2263-2286)
 * are three kernels + the two search kernels.  Problem p reads the keypoint-indexed arrays of the current frame at element
 * offset p * frame_stride (live counts d_frame_n[p * frame_n_stride], or cur0->n when d_frame_n is NULL) and the arrays of
 * orbm_last_frame_t at element offset p * last_stride (live counts d_last_n[p * last_n_stride] or last0->n); Tcw / Tlw hold
 * 16 floats per problem.  scale_factors / cam_params are HOST arrays (copied into the kernel arguments).
 * d_slot / d_slot_obs [npairs][frame_stride] in/out as in orbm_search_by_projection; d_match_of_query [npairs][last_stride]
 * (out, may be NULL) = current-frame keypoint matched by last-frame keypoint i after pruning, or -1; d_nmatches[npairs] out. */
typedef struct {
  int32_t n;                        /* nLast when d_last_n is NULL */
  const uint8_t *has_mp;            /* LastFrame.mvpMapPoints[i] && !LastFrame.mvbOutlier[i] */
  const float *Xw;                  /* 3 floats per keypoint */
  const uint8_t *mpdesc;            /* 32 bytes per keypoint */
  const orbx_keypoint_t *last_keys; /* octave (mvKeys) and angle (mvKeysUn: the same value) */
  const uint8_t *obs;               /* or NULL = all 1 */
  const float *Tcw, *Tlw;           /* row-major 4x4 per problem */
} orbm_last_frame_t;
int orbm_search_by_projection_last_frame_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                                      int frame_n_stride, const orbm_last_frame_t *last0, int last_stride,
                                                      const int32_t *d_last_n, int last_n_stride, int npairs, const float *scale_factors,
                                                      int nlevels, int cam_type, const float *cam_params, float mb, float mbf, float th,
                                                      int bMono, int checkOri, int32_t *d_slot, uint8_t *d_slot_obs,
                                                      int32_t *d_match_of_query, int32_t *d_nmatches, void *stream);

/* void Tracking::SearchLocalPoints()  (Tracking.cc:3449-3539, Frame::Nleft == -1) after its first loop (the frame's own points
 * marked, :3453-3471): Frame::isInFrustum(pMP, viewing_cos_limit) (Frame.cc:572-661) for every local map point, then
 * int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, bFarPoints, thFarPoints)
 * (ORBmatcher.cc:44-143) over the same points, all on the device.  MapPoint::PredictScale (MapPoint.cc:587-602) goes through
 * the bit-exact replica of glibc's logf (csrc/orb_logf.h, orbx_ref_logf).
 * Local map point i, problem p at element offset p * map_stride (Tracking::mvpLocalMapPoints, flattened): */
typedef struct {
  int32_t n;                        /* mvpLocalMapPoints.size(); the live count when d_map_n is NULL */
  const uint8_t *eligible;          /* !pMP->isBad() && pMP->mnLastFrameSeen != CurrentFrame.mnId (Tracking.cc:3455-3468, :3483-3487) */
  const float *Xw;                  /* pMP->GetWorldPos(), 3 floats per point (Frame.cc:581) */
  const float *normal;              /* pMP->GetNormal(), 3 floats per point (Frame.cc:620) */
  const float *max_dist, *min_dist; /* raw mfMaxDistance / mfMinDistance: the 1.2 / 0.8 factors of GetMax/MinDistanceInvariance
                                       (MapPoint.cc:555-565) and PredictScale's ratio (MapPoint.cc:593) are applied inside */
  const uint8_t *mpdesc;            /* pMP->GetDescriptor(), 32 bytes per point (ORBmatcher.cc:76) */
  const uint8_t *obs;               /* pMP->Observations() > 0 (ORBmatcher.cc:89-91), or NULL = all 1 */
  const float *Tcw;                 /* CurrentFrame.mTcw (the pose after Optimizer::PoseOptimization), row-major 4x4 per problem */
} orbm_local_map_t;
/* What isInFrustum writes into the MapPoint, per local map point (same indexing, caller arrays).  Eligible points: in_view =
 * mbTrackInView (Frame.cc:576, :635), proj_x / proj_y = mTrackProjX / Y (-1 unless the projection is inside the image bounds,
 * :577-578, :605-606), and where in_view is set proj_xr = mTrackProjXR = u - mbf / z, depth = mTrackDepth = |Pc|,
 * level = mnTrackScaleLevel, view_cos = mTrackViewCos (:636-644); the other fields of an eligible point and every field but
 * in_view = 0 of an ineligible one are left as they were. */
typedef struct {
  uint8_t *in_view;
  float *proj_x, *proj_y, *proj_xr, *depth, *view_cos;
  int32_t *level;
} orbm_track_t;
/* Host pointers.  cur: the current frame (u_right = mvuRight or NULL; bounds mnMinX..mnMaxY); scale_factors /
 * log_scale_factor / nlevels = mvScaleFactors / mfLogScaleFactor / mnScaleLevels; cam_type / cam_params as in orbm_project;
 * mbf = CurrentFrame.mbf; viewing_cos_limit = 0.5 in the reference (Tracking.cc:3490); th, bFarPoints, thFarPoints, nnratio as
 * passed to SearchByProjection (th picked at Tracking.cc:3509-3534, nnratio 0.8 at :3508).  A map point takes part in the
 * search iff it is in view, eligible and not a far point (:52-59); the window is RadiusByViewingCos(mTrackViewCos) (x th when
 * th != 1) x mvScaleFactors[level], levels [level - 1, level] (:63-73); with u_right, the right-coordinate check uses proj_xr
 * (:93-98).  Claims are sequential in local-map order; slot / slot_obs (in/out) as in orbm_search_by_projection (the frame's
 * mvpMapPoints after the last-frame / reference-keyframe search and the outlier removal).  match_of_point[n] (out, may be
 * NULL) = keypoint matched by local map point i or -1.  One staged upload, the projection kernel and the search kernels, one
 * download, one synchronisation.  Returns nmatches; ORBX_E_ARG for nlevels outside [1, 16], cam_type not 0 / 1, a missing
 * required pointer (every field of map but obs, every field of track, slot, slot_obs) or a frame above ORBM_MAX_KEYPOINTS. */
int orbm_search_local_points(orbm_t *m, const orbm_frame_t *cur, const float *scale_factors, int nlevels, float log_scale_factor,
                             const orbm_local_map_t *map, int cam_type, const float *cam_params, float mbf, float viewing_cos_limit,
                             float th, int bFarPoints, float thFarPoints, float nnratio, int32_t *slot, uint8_t *slot_obs,
                             int32_t *match_of_point, const orbm_track_t *track);
/* Batched device form: `npairs` independent (current frame, local map) problems resident in HBM, asynchronous on `stream`,
 * nothing touches the host.  The keypoint-indexed arrays of problem p at element offset p * frame_stride (live counts
 * d_frame_n[p * frame_n_stride], or cur0->n when d_frame_n is NULL), the arrays of map0 and track0 at element offset
 * p * map_stride (live counts d_map_n[p * map_n_stride], or map0->n), Tcw 16 floats per problem.  scale_factors / cam_params
 * are HOST arrays (copied into the kernel arguments).  d_slot / d_slot_obs [npairs][frame_stride] in/out,
 * d_match_of_point [npairs][map_stride] (out, may be NULL), d_nmatches[npairs] out.  The search windows only exist after the
 * projection kernel has run, so walk or scan is voted per problem on the device (unless orbm_set_scan_mode forces it).
 * ORBX_E_ARG as the host form, and when map_stride / frame_stride is below map0->n / cur0->n without device counts. */
int orbm_search_local_points_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                          int frame_n_stride, const orbm_local_map_t *map0, int map_stride, const int32_t *d_map_n,
                                          int map_n_stride, int npairs, const float *scale_factors, int nlevels, float log_scale_factor,
                                          int cam_type, const float *cam_params, float mbf, float viewing_cos_limit, float th,
                                          int bFarPoints, float thFarPoints, float nnratio, int32_t *d_slot, uint8_t *d_slot_obs,
                                          int32_t *d_match_of_point, const orbm_track_t *track0, int32_t *d_nmatches, void *stream);

/* The same two members for a fisheye-stereo frame (Frame::Nleft != -1): ORBmatcher.cc:44-214 with its second half
 * (:145-211, right camera) and ORBmatcher.cc:2027-2289 with its extra pass (:2189-2256).
 * frame: n = Nleft + Nright; keys_un = mvKeys followed by mvKeysRight (raw keypoints: GetFeaturesInArea reads mvKeys /
 * mvKeysRight when Nleft != -1, Frame.cc:791-793), descriptors = mDescriptors (vconcat of both images, Frame.cc
 * fisheye ctor), u_right = NULL; slot / slot_obs have n entries (F.mvpMapPoints; right keypoint j is entry Nleft + j).
 * left_to_right[Nleft] / right_to_left[Nright] = mvLeftToRightMatch / mvRightToLeftMatch (index in the other image
 * or -1; NULL = none): an accepted match also writes the partner's slot (:128-132, :199-203).
 * Queries: TWO per map point, query 2j = left image (mTrackProjX/Y, mnTrackScaleLevel, mbTrackInView), query 2j+1 =
 * right image (mTrackProjXR/YR, mnTrackScaleLevelR, mbTrackInViewR && level != -1); radius as in
 * orbm_queries_t (the right half does not multiply by th, :148).  The reference's `continue` at :125 (left ratio
 * test failed => right half skipped) is applied inside.  Returns nmatches including the partner increments. */
int orbm_search_by_projection_fisheye(orbm_t *m, const orbm_frame_t *frame, int n_left, const int32_t *left_to_right,
                                      const int32_t *right_to_left, const orbm_queries_t *q, float nnratio, int th_dist,
                                      int32_t *slot, uint8_t *slot_obs, int32_t *match_of_query, int32_t *best_dist);
/* Trl = CurrentFrame.mTrl (row-major 3x4 or 4x4, row stride 4).  slot values are last-frame indices i.  The right
 * pass of a map point is skipped when its left window is empty (:2126).  One staged upload, the kernels of the batched form
 * below with npairs = 1 (projection of both cameras, search, slot conversion and rotation pruning on the device), one
 * download, one synchronisation.  ORBX_E_ARG also for nlevels outside [1, 16] and for a point with has_mp whose octave is
 * outside [0, nlevels). */
int orbm_search_by_projection_last_frame_fisheye(orbm_t *m, const orbm_frame_t *cur, int n_left, const float *scale_factors,
                                                 int nlevels, int nLast, const uint8_t *has_mp, const float *Xw,
                                                 const uint8_t *mpdesc, const orbx_keypoint_t *last_keys, const uint8_t *obs,
                                                 const float *Tcw, const float *Tlw, const float *Trl, int cam_type,
                                                 const float *cam_params, float mb, float th, int bMono, int checkOri,
                                                 int32_t *slot, uint8_t *slot_obs);

/* The Frame of a two-camera fisheye rig from two resident extractions: Frame.cc:1162-1164 (N = Nleft + Nright, mvKeys and
 * mvKeysRight as the searches address them: keypoint k < Nleft is mvKeys[k], the others mvKeysRight[k - Nleft]) and :1201
 * (mDescriptors = vconcat(mDescriptors, mDescriptorsRight)).  No handle: device pointers, asynchronous on `stream`, no host
 * synchronisation, copy or allocation.  d_keysL / d_descL / d_countsL and d_keysR / d_descR / d_countsR are what two
 * orbx_extract_batch_device calls of the same cap wrote ([nframes][cap], [nframes][cap][32], [nframes][2]; the descriptors
 * 16-byte aligned).  Per frame f with nL = d_countsL[2 f], nR = d_countsR[2 f] (each taken as 0 below 0 and cap above cap):
 * d_keys [nframes][2 * cap] and d_desc [nframes][2 * cap][32] receive the nL left entries and the nR right entries directly
 * behind them; entries beyond nL + nR are left alone; d_n [nframes][2] = {nL + nR, nL}, which is what the search below reads
 * as d_frame_n and d_n_left with stride 2.  One kernel: descriptors as 16-byte accesses, keypoints (28 bytes, the right
 * image's at an offset that is a multiple of 4 only) as dwords.
 * ORBX_E_ARG: a NULL pointer, nframes < 0 or above 65535, cap <= 0, 2 * cap above ORBM_FISHEYE_MAX_KEYPOINTS.  nframes == 0
 * returns 0 and launches nothing.  Returns 0, ORBX_E_ARG or ORBX_E_HIP. */
int orbm_rig_concat_batch_device(int nframes, const orbx_keypoint_t *d_keysL, const uint8_t *d_descL, const int32_t *d_countsL,
                                 const orbx_keypoint_t *d_keysR, const uint8_t *d_descR, const int32_t *d_countsR, int cap,
                                 orbx_keypoint_t *d_keys, uint8_t *d_desc, int32_t *d_n, void *stream);

/* ---- Frame::ComputeStereoFishEyeMatches (Frame.cc:1228-1268) ----
 * The arithmetic, one host/device definition each (csrc/orb_ref_triangulate.h); cameras are KannalaBrandt8 parameter sets
 * {fx, fy, cx, cy, k0..k3}, Tlr = [mRlr | mtlr] as 12 floats with row stride 4 (a host array, like Trl of the other rig calls).
 * orbm_unproject: KannalaBrandt8::unproject (KannalaBrandt8.cpp:112-139) of n pixels xy [n][2] into rays [n][3].  Host only.
 * orbm_fisheye_ratio_test: Lowe's test of Frame.cc:1253 on two Hamming distances, `(float)d0 < (float)d1 * 0.7` in double.
 * orbm_fisheye_triangulate: KannalaBrandt8::TriangulateMatches (:343-412) of n keypoint pairs kp1 / kp2 [n][2] with
 * sigma1[i] / sigma2[i] = mvLevelSigma2 of their octaves: depth[i] = z1 or -1, p3D [n][3] written where the function reaches its
 * end.  No GPU call.  cv::SVD is restated as OpenCV's own float one-sided Jacobi [OPENCV-UNVERIFIED].
 * orbm_fisheye_triangulate_device: the same over device arrays, asynchronous on `stream`.
 * All return 0 or ORBX_E_ARG (a NULL pointer, n < 0), the device form also ORBX_E_HIP. */
int orbm_unproject(const float *cam_params, int n, const float *xy, float *rays);
int orbm_fisheye_ratio_test(int d0, int d1);
int orbm_fisheye_triangulate(int n, const float *kp1, const float *kp2, const float *sigma1, const float *sigma2, const float *Tlr,
                             const float *cam_params, const float *cam_params2, float *depth, float *p3D);
int orbm_fisheye_triangulate_device(int n, const float *d_kp1, const float *d_kp2, const float *d_sigma1, const float *d_sigma2, const float *Tlr,
                                    const float *cam_params, const float *cam_params2, float *d_depth, float *d_p3D, void *stream);

/* The whole member for `nframes` resident rig frames: asynchronous on `stream`, no host synchronisation, copy or allocation beyond
 * growth of the handle's scratch (8 bytes per frame and cap entry).  d_keysL .. d_countsR are what two orbx_extract_batch_device
 * calls of the same cap wrote; d_counts[f] = {N, monoIndex}, taken into [0, cap] and [0, N]; the lapping rows are [monoIndex, N)
 * (Frame.cc:1230-1234).  level_sigma2 [nlevels] = mvLevelSigma2, Tlr and both parameter sets are host arrays.
 * Outputs, `out_stride` entries per frame (2 * cap feeds orbm_search_local_points_fisheye_batch_device directly):
 *   d_left_to_right[0 .. Nleft), d_right_to_left[0 .. Nright): index in the other image or -1; where several accepted left
 *     keypoints share a right one, the right one keeps the last in left order (the reference's loop is sequential);
 *   d_depth[0 .. Nleft) = mvDepth, -1.0f where unmatched (the d_depth of orbx_close_points_batch_device);
 *   d_p3d [..][3] = mvStereo3Dpoints, written only where matched;
 *   d_nmatches [nframes][2] = {nMatches, descMatches}, may be NULL.
 * Live entries are reset before any match is written; entries beyond them are left alone.  A frame without a left lapping row or
 * with fewer than two right lapping rows has no matches.  A keypoint octave outside [0, nlevels) makes its pair a non-match.
 * Two kernels: knnMatch(k = 2) on the matrix pipe, one grid over all frames; ratio test + TriangulateMatches, one match per lane.
 * ORBX_E_ARG: a NULL required pointer, nframes outside [0, 65535], cap <= 0, 2 * cap above ORBM_FISHEYE_MAX_KEYPOINTS,
 * out_stride < cap, nlevels outside [1, 16].  nframes == 0 returns 0 and launches nothing. */
int orbm_stereo_fisheye_matches_batch_device(orbm_t *m, int nframes, const orbx_keypoint_t *d_keysL, const uint8_t *d_descL, const int32_t *d_countsL,
                                             const orbx_keypoint_t *d_keysR, const uint8_t *d_descR, const int32_t *d_countsR, int cap,
                                             const float *level_sigma2, int nlevels, const float *Tlr, const float *cam_params,
                                             const float *cam_params2, int out_stride, int32_t *d_left_to_right, int32_t *d_right_to_left,
                                             float *d_depth, float *d_p3d, int32_t *d_nmatches, void *stream);
/* One frame from host pointers: one staged upload, the same kernels with nframes = 1, one download, one synchronisation on the
 * handle's stream.  keysL / descL: mvKeys / mDescriptors (nL rows, lapping from monoL), likewise the right image; the outputs have
 * nL, nR, nL and nL * 3 entries (p3d is in/out: unmatched entries keep the caller's values); nmatches [2] may be NULL.
 * ORBX_E_ARG also for a lapping keypoint whose octave is outside [0, nlevels). */
int orbm_stereo_fisheye_matches(orbm_t *m, const orbx_keypoint_t *keysL, const uint8_t *descL, int nL, int monoL, const orbx_keypoint_t *keysR,
                                const uint8_t *descR, int nR, int monoR, const float *level_sigma2, int nlevels, const float *Tlr,
                                const float *cam_params, const float *cam_params2, int32_t *left_to_right, int32_t *right_to_left, float *depth,
                                float *p3d, int32_t *nmatches);

/* Batched device form of orbm_search_by_projection_last_frame_fisheye (ORBmatcher.cc:2027-2289 for CurrentFrame.Nleft != -1,
 * with the right-camera pass :2189-2256): `npairs` independent (current rig frame, last frame) problems, everything resident
 * in HBM, asynchronous on `stream`, nothing touches the host.  Structs, strides and live counts as in
 * orbm_search_by_projection_last_frame_batch_device, with these differences:
 * cur0: keys_un = the concatenated RAW keypoints [mvKeys ; mvKeysRight], descriptors = mDescriptors, as the per-frame form;
 * u_right is ignored (:2139).  N of problem p = d_frame_n[p * frame_n_stride] (or cur0->n), Nleft = d_n_left[p *
 * n_left_stride] (taken into [0, N]), or the constant n_left when d_n_left is NULL; d_n of orbm_rig_concat_batch_device feeds both with stride 2.
 * last0->last_keys = the last frame's concatenated keypoints: octave (:2100-2101) and angle (:2169-2171) of point i.
 * Trl = CurrentFrame.mTrl, row-major with row stride 4 (12 or 16 floats), a HOST array like scale_factors and cam_params.
 * Device work: k_lastframe_project_rig makes the queries 2i (left image: the arithmetic of the monocular form) and 2i + 1
 * (right image: x3Dr = Rrl * x3Dc + trl projected with the frame's own camera, :2190-2192; same radius and level window,
 * :2197-2207; no bounds or depth test; a point the left half drops - invzc < 0, outside the bounds, !has_mp, an octave
 * outside [0, nlevels) - makes neither), their side bytes and descriptors; the search kernels with the image restriction per
 * query and the rule that an empty left window drops the right pass (:2126); k_rot_prune with two queries per point: the
 * slots the search wrote become last-frame indices i (a keypoint's holder is the LAST query that matched it), then the
 * rotation histogram gets one entry per accepted query (:2185, :2252) and every pruned entry decrements nmatches
 * (:2281-2282), so a keypoint matched by two queries counts twice, as in the reference.
 * d_slot / d_slot_obs [npairs][frame_stride] in/out (entries the call does not write keep the caller's values),
 * d_match_of_query [npairs][2 * last_stride] (out, may be NULL): entry 2i = the left-image match of last point i, 2i + 1 its
 * right-image match, indices into the concatenated frame or -1, after pruning.  d_nmatches[npairs] out.
 * ORBX_E_ARG: what the monocular batch form refuses (npairs < 0 here), NULL Trl, a constant n_left outside [0, cur0->n],
 * frame_stride above ORBM_FISHEYE_MAX_KEYPOINTS.  npairs == 0 returns 0 and launches nothing. */
int orbm_search_by_projection_last_frame_fisheye_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                                              int frame_n_stride, const int32_t *d_n_left, int n_left_stride, int n_left,
                                                              const orbm_last_frame_t *last0, int last_stride, const int32_t *d_last_n,
                                                              int last_n_stride, int npairs, const float *scale_factors, int nlevels,
                                                              const float *Trl, int cam_type, const float *cam_params, float mb, float th,
                                                              int bMono, int checkOri, int32_t *d_slot, uint8_t *d_slot_obs,
                                                              int32_t *d_match_of_query, int32_t *d_nmatches, void *stream);

/* void Tracking::SearchLocalPoints() for a fisheye-stereo frame (Frame::Nleft != -1): Frame::isInFrustum's else branch
 * (Frame.cc:650-660), i.e. Frame::isInFrustumChecks (Frame.cc:1270-1343) once per camera with MapPoint::PredictScale
 * (MapPoint.cc:587-602), then both halves of SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
 * (ORBmatcher.cc:44-214), all on the device.
 * What the frustum test writes per local map point (caller arrays, indexed like orbm_local_map_t).  An eligible point gets
 * in_view = in_view_r = 0 and level = level_r = -1 first (Frame.cc:651-654); then a side whose checks all pass gets its five
 * fields - left (:1335-1339): proj_x, proj_y, level, view_cos, depth = |Pc|; right (:1328-1332): proj_xr, proj_yr, level_r,
 * view_cos_r, depth_r - and its flag (:656-657).  There is no reset of the projection to -1 in this branch: the fields of a side
 * that fails keep the caller's values.  An ineligible point gets in_view = in_view_r = 0 and nothing else.
 * depth is IN/OUT: the far-point test (ORBmatcher.cc:56) reads mTrackDepth, the LEFT depth, as it stands after the frustum step,
 * so for a point whose left check fails and whose right check passes it reads the value the caller passed in. */
typedef struct {
  uint8_t *in_view, *in_view_r;                      /* mbTrackInView, mbTrackInViewR */
  float *proj_x, *proj_y, *depth, *view_cos;         /* mTrackProjX / Y, mTrackDepth, mTrackViewCos */
  float *proj_xr, *proj_yr, *depth_r, *view_cos_r;   /* mTrackProjXR / YR, mTrackDepthR, mTrackViewCosR */
  int32_t *level, *level_r;                          /* mnTrackScaleLevel, mnTrackScaleLevelR */
} orbm_track_rig_t;
/* Host pointers.  cur as in orbm_search_by_projection_fisheye: keys_un = the RAW keypoints [mvKeys ; mvKeysRight], descriptors =
 * mDescriptors, n = Nleft + Nright, u_right ignored (ORBmatcher.cc:93); one set of bounds for both cameras (Frame.cc:1302-1305).
 * left_to_right[n_left] / right_to_left[n - n_left] = mvLeftToRightMatch / mvRightToLeftMatch (NULL = none).  map: unchanged.
 * Trl = mTrl, row-major with row stride 4 (12 or 16 floats); tlr = mTlr.col(3).  The right camera is mR = Rrl * mRcw,
 * mt = Rrl * mtcw + trl, twc = mRwc * tlr + mOw (Frame.cc:1276-1280).  cam_type / cam_params = mpCamera projects the left side,
 * cam_type2 / cam_params2 = mpCamera2 the right side (Frame.cc:1299-1300; the last-frame search uses mpCamera for both).
 * A point takes part iff it is eligible, in_view || in_view_r (ORBmatcher.cc:53) and not a far point (:56, see depth above).
 * Left query (:62-73) where in_view: radius RadiusByViewingCos(view_cos) (x th when th != 1) x mvScaleFactors[level], levels
 * [level - 1, level], left keypoints.  Right query (:145-151) where in_view_r && level_r != -1: RadiusByViewingCos(view_cos_r)
 * WITHOUT th (:148) x mvScaleFactors[level_r] around (proj_xr, proj_yr), right keypoints.  A NaN projection makes no query.  A left
 * half that fails the ratio test drops the right half (:127); an empty left window does not (:75).  An accepted match also writes
 * its stereo partner's slot, unconditionally, and counts it (:132-136, :199-203).  Claims are sequential in local-map order, left
 * half before right half.  slot / slot_obs [n] in/out: slots this call writes hold local-map indices i.  match_of_point[2 nmp]
 * (out, may be NULL): entry 2i the left match of point i, 2i + 1 its right match, indices into the concatenated frame or -1.
 * One staged upload, the kernels of the batched form below with npairs = 1, one download, one synchronisation; a frame without
 * keypoints still gets its track fields.  Returns nmatches including the partner increments.  ORBX_E_ARG as
 * orbm_search_local_points, and for NULL Trl / tlr / cam_params2, cam_type2 not 0 / 1, n_left outside [0, n], n above
 * ORBM_FISHEYE_MAX_KEYPOINTS, a partner index beyond the other image's count. */
int orbm_search_local_points_fisheye(orbm_t *m, const orbm_frame_t *cur, int n_left, const int32_t *left_to_right,
                                     const int32_t *right_to_left, const float *scale_factors, int nlevels, float log_scale_factor,
                                     const orbm_local_map_t *map, const float *Trl, const float *tlr, int cam_type,
                                     const float *cam_params, int cam_type2, const float *cam_params2, float viewing_cos_limit, float th,
                                     int bFarPoints, float thFarPoints, float nnratio, int32_t *slot, uint8_t *slot_obs,
                                     int32_t *match_of_point, const orbm_track_rig_t *track);
/* Batched device form: layout, strides and live counts as in orbm_search_local_points_batch_device; d_n_left / n_left_stride /
 * n_left as in orbm_search_by_projection_last_frame_fisheye_batch_device (d_n of orbm_rig_concat_batch_device feeds d_frame_n and
 * d_n_left with stride 2).  d_left_to_right / d_right_to_left [npairs][frame_stride] (either may be NULL): the first Nleft resp.
 * N - Nleft entries of a problem are live; an entry outside the other image's live range counts as -1 (ORBmatcher.cc:132, :199;
 * the per-frame form refuses it).  d_match_of_point [npairs][2 * map_stride] (out, may be NULL); the arrays of track0 at element
 * offset p * map_stride; Trl, tlr, both cam_params and scale_factors are HOST arrays.  Device work: k_local_map_project_rig (both
 * frustum tests, the queries 2i / 2i + 1 with side bytes and descriptors, the partner table), the search kernels with the image
 * restriction per query, the :127 rule and the partner writes, k_rig_slot_convert (query ids in the written slots, partner slots
 * included, become local-map indices; a slot's holder is the LAST query that wrote it).  With partner tables AND map0->obs the
 * claims are resolved one query at a time (a partner write of a point without observations can release a claim, and whether such
 * a point exists is only known on the device); the result is exact in either mode.  Entries the call does not write, in every
 * array, keep the caller's values.  Asynchronous on `stream`: no host synchronisation, copy or allocation beyond the growth of the
 * handle's scratch.  ORBX_E_ARG as orbm_search_local_points_batch_device (npairs < 0 here) and as the per-frame form, and for
 * frame_stride above ORBM_FISHEYE_MAX_KEYPOINTS.  npairs == 0 returns 0 and launches nothing. */
int orbm_search_local_points_fisheye_batch_device(orbm_t *m, const orbm_frame_t *cur0, int frame_stride, const int32_t *d_frame_n,
                                                  int frame_n_stride, const int32_t *d_n_left, int n_left_stride, int n_left,
                                                  const int32_t *d_left_to_right, const int32_t *d_right_to_left,
                                                  const orbm_local_map_t *map0, int map_stride, const int32_t *d_map_n, int map_n_stride,
                                                  int npairs, const float *scale_factors, int nlevels, float log_scale_factor,
                                                  const float *Trl, const float *tlr, int cam_type, const float *cam_params, int cam_type2,
                                                  const float *cam_params2, float viewing_cos_limit, float th, int bFarPoints,
                                                  float thFarPoints, float nnratio, int32_t *d_slot, uint8_t *d_slot_obs,
                                                  int32_t *d_match_of_point, const orbm_track_rig_t *track0, int32_t *d_nmatches, void *stream);
/* The right camera of isInFrustumChecks (Frame.cc:1276-1280) as the kernels form it, host: Tr[12] = [Rrl * mRcw | Rrl * mtcw + trl]
 * (row stride 4), twc[3] = mRwc * tlr + mOw.  Tcw: row-major 4x4; Trl: row stride 4. */
void orbm_rig_right_camera(const float *Tcw, const float *Trl, const float *tlr, float *Tr, float *twc);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound,
 *                                    const float th, const int ORBdist)                       (ORBmatcher.cc:2291-2413)
 * flattened, host pointers.  i in [0, nKF): valid[i] = pMP && !pMP->isBad() && !sAlreadyFound.count(pMP);
 * Xw = GetWorldPos(); mpdesc = GetDescriptor(); kf_angle[i] = pKF->mvKeysUn[i].angle; max_dist / min_dist =
 * MapPoint::mfMaxDistance / mfMinDistance (the 1.2 / 0.8 invariance factors of MapPoint.cc:552-563 and PredictScale,
 * MapPoint.cc:587-602, are applied inside).  log_scale_factor = CurrentFrame.mfLogScaleFactor.  Every occupied slot
 * blocks (:2355-2356): pass slot_obs = 1 for all occupied keypoints.  Returns nmatches after the rotation check. */
int orbm_search_by_projection_keyframe(orbm_t *m, const orbm_frame_t *cur, const float *scale_factors, int nlevels,
                                       float log_scale_factor, int nKF, const uint8_t *valid, const float *Xw,
                                       const uint8_t *mpdesc, const float *kf_angle, const float *max_dist,
                                       const float *min_dist, const float *Tcw, int cam_type, const float *cam_params,
                                       float th, int ORBdist, int checkOri, int32_t *slot, uint8_t *slot_obs);

/* int ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints,
 *                                    vector<MapPoint*> &vpMatched, int th, float ratioHamming)   (ORBmatcher.cc:489-602)
 * and its :604-720 overload (which only stores one more pointer per match), flattened, host pointers.
 * kf = the keyframe's mvKeysUn / mDescriptors / image bounds; i in [0, nP): valid[i] = !pMP->isBad() &&
 * !spAlreadyFound.count(pMP); Xw = GetWorldPos(); normal = GetNormal(); max_dist / min_dist = mfMaxDistance /
 * mfMinDistance; Scw row-major 4x4 (Sim3); cam = {fx, fy, cx, cy}; log_scale_factor = pKF->mfLogScaleFactor.
 * slot (in/out) = vpMatched as candidate-point index or -1; every occupied slot blocks (:577-578).  Returns nmatches. */
int orbm_search_by_projection_sim3(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, int nlevels,
                                   float log_scale_factor, int nP, const uint8_t *valid, const float *Xw,
                                   const float *normal, const uint8_t *mpdesc, const float *max_dist,
                                   const float *min_dist, const float *Scw, const float *cam, int th,
                                   float ratioHamming, int32_t *slot, uint8_t *slot_obs);

/* The same member for any camera model of the keyframe (pKF->mpCamera->project, :534): cam_type / cam_params as in orbm_project.
 * orbm_search_by_projection_sim3 is this with cam_type 0. */
int orbm_search_by_projection_sim3_cam(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, int nlevels, float log_scale_factor, int nP,
                                       const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc,
                                       const float *max_dist, const float *min_dist, const float *Scw, int cam_type, const float *cam_params,
                                       int th, float ratioHamming, int32_t *slot, uint8_t *slot_obs);

/* int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th, const bool bRight = false)
 *                                                                                             (ORBmatcher.cc:1425-1658)
 * kf = the keyframe's mvKeysUn / mDescriptors / mvuRight (NULL = all -1) / image bounds; i in [0, nP): valid[i] =
 * pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF); Xw = GetWorldPos(), normal = GetNormal(), mpdesc = GetDescriptor(),
 * max_dist / min_dist = mfMaxDistance / mfMinDistance (the 1.2 / 0.8 invariance factors are applied inside);
 * Tcw = row-major 4x4 [GetRotation() | GetTranslation()], Ow = GetCameraCenter(); cam as in orbm_project; bf = pKF->mbf.
 * The search of one map point does not depend on the others, so the function returns the per-point result -
 * best_idx[i] = keypoint (bestDist <= TH_LOW) or -1, best_dist[i] - and the caller applies :1622-1640 (Replace /
 * AddObservation / AddMapPoint) on its objects in index order.  Returns nFused = #{i : best_idx[i] >= 0}. */
int orbm_fuse(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, const float *inv_level_sigma2, int nlevels,
              float log_scale_factor, int nP, const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc,
              const float *max_dist, const float *min_dist, const float *Tcw, const float *Ow, int cam_type, const float *cam_params,
              float bf, float th, int32_t *best_idx, int32_t *best_dist);
/* int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th,
 *                      vector<MapPoint*> &vpReplacePoint)                                      (ORBmatcher.cc:1660-1786)
 * valid[i] = !pMP->isBad() && !spAlreadyFound.count(pMP); Scw row-major 4x4 (Sim3); cam = {fx, fy, cx, cy}. */
int orbm_fuse_sim3(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, int nlevels, float log_scale_factor, int nP,
                   const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc, const float *max_dist,
                   const float *min_dist, const float *Scw, const float *cam, float th, int32_t *best_idx, int32_t *best_dist);

/* ... for any camera model (pKF->mpCamera->project, :1704); orbm_fuse_sim3 is this with cam_type 0. */
int orbm_fuse_sim3_cam(orbm_t *m, const orbm_frame_t *kf, const float *scale_factors, int nlevels, float log_scale_factor, int nP,
                       const uint8_t *valid, const float *Xw, const float *normal, const uint8_t *mpdesc, const float *max_dist,
                       const float *min_dist, const float *Scw, int cam_type, const float *cam_params, float th, int32_t *best_idx,
                       int32_t *best_dist);

/* ---- LocalMapping::SearchInNeighbors (LocalMapping.cc:909-1058): ONE list of map points fused into ALL target keyframes per call ----
 * The reference calls ORBmatcher::Fuse(pKFi, vpMapPointMatches) once per target keyframe (:989-1000; a rig keyframe twice, the second
 * time with bRight = true), always with the same points, and then once in the other direction (:1033-1035).  orbm_fuse_keyframes is
 * the search part of all those calls: the point arrays are uploaded once, the T keyframes and the valid table in the same block, one
 * kernel (k_fuse_keyframes: gates, window, chi-square gate and Hamming search on the device), one download of the two tables, one
 * synchronisation.
 *
 * One target = what orbm_fuse takes of a keyframe. */
typedef struct {
  orbm_frame_t kf;                 /* what the search reads of the keyframe: mvKeysUn / mDescriptors / mvuRight / bounds; for a rig the raw
                                      keypoints and descriptor rows of ONE image (mvKeys, or mvKeysRight with the rows behind NLeft) */
  const float *scale_factors;      /* mvScaleFactors [nlevels] */
  const float *inv_level_sigma2;   /* mvInvLevelSigma2 [nlevels] */
  int32_t nlevels;                 /* [1, ORBX_MAX_LEVELS] */
  float log_scale_factor;
  const float *Tcw;                /* row-major 4x4; the right camera's pose for bRight */
  const float *Ow;                 /* [3] */
  int32_t cam_type; const float *cam_params;   /* as in orbm_project; mpCamera2's for bRight */
  float bf;
} orbm_fuse_target_t;

/* valid [T][nP]: row t = valid of orbm_fuse for target t (pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF_t)); Xw, normal, mpdesc,
 * max_dist, min_dist [nP] and th as in orbm_fuse.  Out: best_idx / best_dist [T][nP], nfused [T].
 * Row t is bit for bit what orbm_fuse returns for target t with valid + t * nP, nfused[t] is the return value of that call, and the
 * function returns the sum of nfused.  A right camera of a rig is just another target: the caller adds NLeft to its indices.  Targets
 * may differ in keypoint count, image bounds, camera model, nlevels and scale tables.  A target with kf.n == 0, or a valid row of
 * zeros, gives a row of -1 / 256.  T == 0 or nP == 0 returns 0 and does not touch the device.
 * ORBX_E_ARG, with orbm_last_error naming the target ("target <t>: ...") where there is one, for:
 *   - whatever orbm_fuse refuses (a NULL handle, table, array or result pointer, nP < 0, kf.n < 0, NULL keypoints or descriptors);
 *   - T < 0, or a NULL target table with T > 0;
 *   - kf.n above ORBM_MAX_KEYPOINTS; empty bounds (also where kf.n == 0: the record's grid constants divide by their extent);
 *   - nlevels outside [1, 16]; a keypoint octave outside [0, nlevels), because the kernel indexes device tables with it;
 *   - a cam_type other than 0 or 1.
 *
 * Why the T searches may leave the reference's loop although its body (ORBmatcher.cc:1622-1645) changes map points between them - the
 * FUSE RULE, next to the MASKING RULE and the SEQUENTIAL RULE below:
 *   - Read-only keyframe inputs.  The search reads of a keyframe only keypoints, descriptors, mvuRight, pose, camera and scale tables;
 *     all of these are read-only in the loop.  The search is claimless: a keypoint that has received a map point stays a candidate
 *     (:1622-1640 look at pKF->GetMapPoint(bestIdx) only after the search), so different points never see one another inside a target.
 *   - What the search reads of a point: isBad(), IsInKeyFrame(pKF), world position, normal, the two distances and the descriptor.
 *   - What the loop body changes: it calls MapPoint::Replace (MapPoint.cc:249-301) or AddObservation (+ KeyFrame::AddMapPoint).
 *     Neither changes position, normal or distances.  AddObservation changes only the observations.  Replace makes the loser bad for
 *     good and only ADDS observations to the survivor; it calls the survivor's ComputeDistinctiveDescriptors(), which can change its
 *     descriptor.  The survivor can be the searched point or the keyframe's own point; in the second case it can sit elsewhere in
 *     the list, so the caller tests by content (GetDescriptor() against the uploaded bytes), not by index.
 *   - Validity only shrinks: a bad point stays bad, a point in pKF stays in pKF, so live validity is always a subset of validity at
 *     loop entry.
 *   - The rule.  The sequential result for (t, i) is entry (t, i) of the tables computed from the state at loop entry, used under the
 *     reference's own live test (!isBad() && !IsInKeyFrame(pKF_t)).  The exception is a point whose GetDescriptor() now differs from
 *     the 32 bytes that were uploaded: for those points alone the caller repeats the search of target t, with orbm_fuse on the subset,
 *     at the start of iteration t.  That is early enough, because iteration t itself cannot dirty a point that is still valid for t:
 *     a survivor is in pKF_t afterwards.
 *   - Rigs.  The two targets of one rig keyframe are consecutive; between them the same test applies (the right call's IsInKeyFrame
 *     sees what the left call added).
 *   - How large the dirty fraction is on real sequences is NOT KNOWN here: no sequence was run.  Every dirty point costs one entry of a
 *     per-target orbm_fuse call on the subset; a loop in which most points turn dirty gains nothing over the per-target calls.
 * tests/test_fuse_keyframes_abi.py and tests/test_gpu_fuse_keyframes.py replay the sequential loop against this rule. */
int orbm_fuse_keyframes(orbm_t *m, int T, const orbm_fuse_target_t *targets /*[T]*/, int nP,
                        const uint8_t *valid /*[T][nP]*/, const float *Xw, const float *normal, const uint8_t *mpdesc,
                        const float *max_dist, const float *min_dist, float th,
                        int32_t *best_idx /*[T][nP]*/, int32_t *best_dist /*[T][nP]*/, int32_t *nfused /*[T]*/);

/* ---- LoopClosing::SearchAndFuse (LoopClosing.cc:2631-2670, :2673-2707): ONE list of loop / merge map points fused into ALL corrected
 * keyframes per call ----
 * Both overloads call the Sim3 overload of ORBmatcher::Fuse (ORBmatcher.cc:1664-1786) once per corrected keyframe (CorrectLoop :1376,
 * the two map merges :1995, :2506), always with the same point list and each time with another Scw.  orbm_fuse_sim3_keyframes is the
 * search part of all those calls, staged and launched as orbm_fuse_keyframes is: the point arrays once, the valid table, the per-target
 * records and every target's keypoints and descriptors in one block, two kernels (k_fuse_sim3_gate lists the pairs that pass the
 * gates, k_fuse_sim3_search searches the lists), one download of the two tables, one synchronisation.
 *
 * One target = what orbm_fuse_sim3_cam takes of a keyframe. */
typedef struct {
  orbm_frame_t kf;                 /* mvKeysUn / mDescriptors / bounds (u_right is not read: this overload has no stereo term) */
  const float *scale_factors;      /* mvScaleFactors [nlevels] */
  int32_t nlevels;                 /* [1, ORBX_MAX_LEVELS] */
  float log_scale_factor;
  const float *Scw;                /* row-major 4x4 Sim3; a pose (scale 1) for the overload that passes GetPose() (:2686) */
  int32_t cam_type; const float *cam_params;   /* as in orbm_project */
} orbm_fuse_sim3_target_t;

/* valid [T][nP]: row t = valid of orbm_fuse_sim3_cam for target t (!pMP->isBad() && !pKF_t->GetMapPoints().count(pMP)); Xw, normal,
 * mpdesc, max_dist, min_dist [nP] and th as there.  Out: best_idx / best_dist [T][nP], nfused [T].
 * Row t is bit for bit what orbm_fuse_sim3_cam returns for target t with valid + t * nP, nfused[t] is the return value of that call,
 * and the function returns the sum of nfused.  Targets may differ in keypoint count, image bounds, camera model, nlevels and scale
 * tables.  A target with kf.n == 0, or a valid row of zeros, gives a row of -1 / 256.  T == 0 or nP == 0 returns 0 and does not touch
 * the device.  Every Scw is decomposed once on the host exactly as orbm_fuse_sim3_cam decomposes it (ORBmatcher.cc:1672-1677).  A Scw whose scale is
 * zero or not finite is NOT refused, because the per-target entry does not refuse it: its T is then NaN or infinite, no projection
 * passes IsInImage, and the row is -1 / 256 on both sides (the kernel clamps every table index: PredictScale's level to
 * [0, nlevels), the cell window to the grid).
 * ORBX_E_ARG, with orbm_last_error naming the target ("target <t>: ...") where there is one, for what orbm_fuse_keyframes refuses
 * (above) without inv_level_sigma2, Tcw and Ow, and for a NULL Scw.  Everything is validated before anything is staged or launched.
 *
 * Why the T searches may leave the reference's loop although its body changes map points between them - the SEARCH-AND-FUSE RULE,
 * next to the FUSE RULE above.  The loop body differs from SearchInNeighbors': inside call t, ORBmatcher::Fuse does AddObservation /
 * AddMapPoint at once for an empty keypoint (:1776-1780) but only RECORDS an occupied one in vpReplacePoint (:1771-1775);
 * SearchAndFuse then replaces, under mMutexMapUpdate, pRep->Replace(vpMapPoints[i]) for every recorded i (:2654-2665, :2693-2704).
 *   - Read-only keyframe inputs, claimless search: as in the FUSE RULE.  The search reads of a keyframe only keypoints, descriptors,
 *     bounds, camera and scale tables; Scw is a local of the loop.  Two points that pick one keypoint do not see each other.
 *   - Nothing iteration t does reaches its own searches.  AddObservation / AddMapPoint change no searched quantity of any point, and
 *     every Replace of iteration t runs after call t has returned.
 *   - Replace always makes the SEARCHED point vpMapPoints[i] the survivor and the keyframe's own point pRep the loser.  The survivor only
 *     gains observations and keyframe memberships; EraseMapPointMatch / ReplaceMapPointMatch touch only the loser's slots, and the loser
 *     is bad from then on.  Validity here is !isBad() && !spAlreadyFound.count(pMP) with spAlreadyFound = pKF_t->GetMapPoints() taken
 *     at entry of iteration t: a listed point can turn bad (it was the pRep of an earlier keypoint) and can enter a keyframe, never the
 *     reverse, so validity at entry of iteration t is a subset of validity at loop entry.  Position, normal and the two distances
 *     never change.
 *   - The only searched quantity that changes is the survivor's descriptor: Replace ends in ComputeDistinctiveDescriptors()
 *     (MapPoint.cc:300), and the survivor is a searched point.
 *   - The rule.  The sequential result for (t, i) is entry (t, i) of the tables computed from the state at loop entry, used under the
 *     live validity test of iteration t.  The exception is a point whose GetDescriptor() now differs from the 32 bytes that were
 *     uploaded: for those points alone the caller repeats the search of target t at the start of iteration t, with orbm_fuse_sim3_cam
 *     on the subset.  The start of iteration t is early enough by the second item.
 *   - A pointer listed twice needs no special case, nor do two points that pick the same keypoint: the body (:1768-1782) and the
 *     deferred Replace loop run on the live objects exactly as the adapter's ORBmatcher::Fuse and the reference's loop run them; only
 *     the (best_idx, best_dist) they start from come from the tables.
 *   - How large the dirty fraction is on real sequences is NOT KNOWN here: no sequence was run.  In this loop EVERY successful Replace
 *     can dirty a searched point (in SearchInNeighbors only those whose survivor is listed), so it is expected to be larger than
 *     there.  Every dirty point costs one entry of a per-target orbm_fuse_sim3_cam call on the subset; a loop in which most points
 *     turn dirty gains nothing over the per-target calls.
 * tests/test_fuse_sim3_keyframes_abi.py and tests/test_gpu_fuse_sim3_keyframes.py replay the sequential loop against this rule. */
int orbm_fuse_sim3_keyframes(orbm_t *m, int T, const orbm_fuse_sim3_target_t *targets /*[T]*/, int nP,
                             const uint8_t *valid /*[T][nP]*/, const float *Xw, const float *normal, const uint8_t *mpdesc,
                             const float *max_dist, const float *min_dist, float th,
                             int32_t *best_idx /*[T][nP]*/, int32_t *best_dist /*[T][nP]*/, int32_t *nfused /*[T]*/);

/* int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12,
 *                              const cv::Mat &R12, const cv::Mat &t12, const float th)           (ORBmatcher.cc:1788-2012)
 * Per keyframe k: kf_k = mvKeysUn / mDescriptors / image bounds, sf_k = mvScaleFactors, log_sf_k = mfLogScaleFactor,
 * valid_k[i] = pMP && !pMP->isBad() && !vbAlreadyMatched_k[i] (:1813-1826), Xw / mpdesc / max_dist / min_dist of the map point
 * of keypoint i, R_kw / t_kw = GetRotation() / GetTranslation() (row-major 3x3 / 3).  cam1 = {fx, fy, cx, cy} of pKF1 (used
 * for both projections, as in the reference).  matches12[kf1->n] (out) = keypoint of kf2 or -1 for the NEW mutual matches
 * (vpMatches12[i1] = vpMapPoints2[matches12[i1]]).  Returns nFound. */
int orbm_search_by_sim3(orbm_t *m, const orbm_frame_t *kf1, const float *sf1, int nlevels1, float log_sf1, const uint8_t *valid1,
                        const float *Xw1, const uint8_t *mpdesc1, const float *max_dist1, const float *min_dist1, const float *R1w,
                        const float *t1w, const orbm_frame_t *kf2, const float *sf2, int nlevels2, float log_sf2, const uint8_t *valid2,
                        const float *Xw2, const uint8_t *mpdesc2, const float *max_dist2, const float *min_dist2, const float *R2w,
                        const float *t2w, float s12, const float *R12, const float *t12, const float *cam1, float th, int32_t *matches12);

/* The slice of KeyFrame that SearchForTriangulation reads (host pointers).  feature vector = DBoW2::FeatureVector
 * (std::map<NodeId, std::vector<unsigned>>, FeatureVector.h:24-25) flattened in key order: node_id[k] ascending,
 * members of node k = node_idx[node_start[k] .. node_start[k+1]). */
typedef struct {
  int32_t n;
  const orbx_keypoint_t *keys_un;  /* mvKeysUn.data() */
  const uint8_t *descriptors;      /* mDescriptors, n x 32 */
  const float *u_right;            /* mvuRight (negative = monocular keypoint) */
  const uint8_t *has_mappoint;     /* GetMapPoint(i) != NULL */
  int32_t n_nodes;
  const uint32_t *node_id;
  const int32_t *node_start;       /* n_nodes + 1 */
  const int32_t *node_idx;
  const float *scale_factors;      /* mvScaleFactors */
  const float *level_sigma2;       /* mvLevelSigma2 */
  int32_t nlevels;
} orbm_keyframe_t;

/* int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>>&,
 *                                        const bool bOnlyStereo, const bool bCoarse)        (ORBmatcher.cc:981-1222)
 * for two Pinhole keyframes without a second camera (mpCamera2 == NULL; F12 is unused by the reference as well).
 * R?w / t?w = GetRotation() / GetTranslation() (row-major 3x3 / 3), Cw1 = pKF1->GetCameraCenter(),
 * cam? = mvParameters {fx, fy, cx, cy}.  The merge-walk over the two feature vectors and the per-pair fundamental
 * matrix (Pinhole.cpp:143-148, identical for every candidate pair, so formed once) run on the host; the per-node
 * all-pairs Hamming scan with the epipole / epipolar gates runs on the device.  matches12[kf1->n] (out) =
 * vMatches12; the reference's vMatchedPairs is {(i, matches12[i]) : matches12[i] >= 0} in ascending i.
 * Returns nmatches. */
int orbm_search_for_triangulation(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_t *kf2, const float *R1w,
                                  const float *t1w, const float *R2w, const float *t2w, const float *Cw1,
                                  const float *cam1, const float *cam2, int bOnlyStereo, int bCoarse, int checkOri,
                                  int32_t *matches12);

/* The same member for keyframes whose epipolar test is NOT Pinhole's: KannalaBrandt8 cameras and two-camera rigs
 * (pCamera1->epipolarConstrain(pCamera2, kp1, kp2, R12, t12, sigma1, sigma2) is a virtual call, ORBmatcher.cc:1148;
 * KannalaBrandt8's is TriangulateMatches(...) > 0.0001f, a cv::SVD triangulation, KannalaBrandt8.cpp:244-247).  Two forms:
 * orbm_search_for_triangulation_kb8 below runs the whole member on the device when every camera involved is a KannalaBrandt8; for any
 * other camera model the device does everything in front of the predicate and the predicate stays the caller's:
 *
 * orbm_triangulation_candidates: per keypoint idx1 of KF1 without a map point (and, with bOnlyStereo, with mvuRight >= 0) every
 * keypoint idx2 of KF2 in the same vocabulary node that has no map point (:1083), passes the stereo filter (:1088-1090), lies
 * within TH_LOW (:1096) and - when epipole_gate != 0 (the reference: !pKF1->mpCamera2) and neither keypoint is stereo - is not
 * within 10 scaled pixels of the epipole (ep_x, ep_y) = pKF2->mpCamera->project(R2w * Cw1 + t2w) (:992, :1105-1113).
 * CSR: cand_start[kf1->n + 1]; cand_idx2 / cand_dist[cap] hold the lists, each ordered by (distance ascending, position in
 * the node DESCENDING): the reference keeps a running best with "dist > bestDist -> skip" and updates it on <=, so its answer is
 * the LAST minimum among the candidates the predicate accepts = the FIRST entry of this order that it accepts.
 * Rigs: pass u_right all negative (bStereo is false for them, :1059, :1086) and the concatenated [left; right] keypoints.
 * Returns the total number of candidates; if it exceeds cap only cand_start was written - call again with that capacity.
 *
 * orbm_search_for_triangulation_pred: the whole member around a caller-supplied predicate: candidates as above, then per idx1
 * the first listed idx2 with bCoarse || pred(user, idx1, idx2), then the rotation-histogram pruning (:1162-1172, :1191-1207).
 * pred is called on the calling thread, only for pairs that passed every other gate, in list order, and must be pure.
 * matches12[kf1->n] (out) = vMatches12.  Returns nmatches.  The adapter takes this route, with pred = the reference's own
 * epipolarConstrain, only when a camera involved is neither Pinhole nor KannalaBrandt8 (csrc/adapter/ORBmatcher_hip.cc). */
typedef int (*orbm_pair_predicate_t)(void *user, int idx1, int idx2);
int orbm_triangulation_candidates(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_t *kf2, float ep_x, float ep_y,
                                  int epipole_gate, int bOnlyStereo, int32_t *cand_start, int32_t *cand_idx2, int32_t *cand_dist,
                                  int cap);
int orbm_search_for_triangulation_pred(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_t *kf2, float ep_x, float ep_y,
                                       int epipole_gate, int bOnlyStereo, int bCoarse, int checkOri, orbm_pair_predicate_t pred,
                                       void *user, int32_t *matches12);

/* The same member with KannalaBrandt8::epipolarConstrain on the device: orbm_search_for_triangulation_pred with
 * pred = kb8 TriangulateMatches(cam_a, cam_b, kp1, kp2, R12, t12, kf1->level_sigma2[octave1], kf2->level_sigma2[octave2]) > 0.0001f
 * (KannalaBrandt8.cpp:244-247, :343-412; the arithmetic of csrc/orb_ref_triangulate.h, cv::SVD restated as OpenCV's own float Jacobi,
 * [OPENCV-UNVERIFIED]).  One upload, three kernels - candidate lists, the test on EVERY candidate with the minimum accepted key per
 * keypoint of KF1 (= the first accepted entry of the order above), keys to indices - and one download; the rotation-histogram pruning
 * runs on the host afterwards.  bCoarse accepts the first entry of every list without the test.  It is
 * orbm_search_for_triangulation_kb8_neighbours with K = 1 behind its own checks (which already were that entry's checks of a keyframe's
 * arrays, listed below); orbm_last_error carries no "neighbour 0: ".  One text is new: a node_idx of kf1 outside [0, n) in a shared
 * node, which left orbm_last_error as it was, now sets it to "kf1: keypoint index out of range" (the code, ORBX_E_ARG, is the same).
 * n_left? == -1: a keyframe without a second camera - keys_un = mvKeysUn, bStereo = u_right >= 0, the epipole gate (:1105-1113) is on;
 * cams? [1][8] = mpCamera's {fx, fy, cx, cy, k0..k3}; T12 [1][12] = [R12 | t12] (row stride 4) of :1007-1008.
 * n_left? >= 0: a two-camera rig - keys_un = [mvKeys; mvKeysRight], keypoint idx is the right camera's when idx >= n_left, bStereo is false
 * for every keypoint (u_right is not read and may be NULL), no epipole gate; cams? [2][8] = mpCamera, mpCamera2; T12 [4][12] in the order
 * ll, lr, rl, rr of :1011-1019, the pair (bRight1, bRight2) selects cameras and pose (:1115-1145).
 * (ep_x, ep_y) = pKF2->mpCamera->project(R2w * Cw1 + t2w) (:988-993) and T12 are the caller's: the cv::Mat algebra stays outside.
 * Returns nmatches, ORBX_E_HIP, or ORBX_E_ARG for:
 *   - a NULL m, kf1, kf2, cams1, cams2, T12 or matches12, a NULL scale_factors / level_sigma2, and with n > 0 a NULL keys_un,
 *     descriptors, has_mappoint or (n_left == -1) u_right, with n_nodes > 0 a NULL node array;
 *   - exactly one of n_left1 / n_left2 equal to -1 (the reference's R12 would be empty there);
 *   - n < 0 or n_left outside [-1, n];
 *   - nlevels of either keyframe outside [1, ORBX_MAX_LEVELS];
 *   - a keypoint of either keyframe with an octave outside [0, nlevels) (checked on the host before anything is uploaded);
 *   - a feature vector whose node_start decreases or whose node_idx holds an index outside [0, n) (kf1: in a node it shares with kf2);
 *   - a vocabulary node of kf2 with more than 65535 members, or more than 2^31 - 1 keypoint pairs in shared nodes. */
int orbm_search_for_triangulation_kb8(orbm_t *m, const orbm_keyframe_t *kf1, int n_left1, const orbm_keyframe_t *kf2, int n_left2,
                                      float ep_x, float ep_y, const float *cams1, const float *cams2, const float *T12,
                                      int bOnlyStereo, int bCoarse, int checkOri, int32_t *matches12);

/* SearchForTriangulation of ONE keyframe against ALL its neighbours in one call: the loop of LocalMapping::CreateNewMapPoints
 * (LocalMapping.cc:475-583; Tracking::CreateNewMapPoints, Tracking.cc:4288, in localisation mode), which calls the member once per
 * neighbour of the new keyframe.  kf1 is staged once, the neighbours' arrays go up in the same block, the kernels' grid covers every
 * (neighbour, keypoint of kf1, shared node) at once: one upload, one fill, one download of [K][kf1->n], one synchronisation per call.
 *
 * Row j of matches12 [K][kf1->n] is bit for bit what the per-pair entry above returns for (kf1, kf2[j]) with checkOri = 0, and
 * nmatches[j] its return value.  skip[j] != 0 (skip may be NULL) stands for the `continue`s of the baseline tests in front of the
 * search (LocalMapping.cc:544-560): row j is all -1, nmatches[j] = 0, and neighbour j is neither validated nor uploaded.
 * Returns the sum of nmatches (K == 0 or every neighbour skipped: 0, without touching the device), ORBX_E_HIP or ORBX_E_ARG.
 *
 * Why the searches may leave the reference's loop although its body changes kf1 between them - the MASKING RULE:
 *   - the loop body gives keypoints of kf1 a map point, mpCurrentKeyFrame->AddMapPoint(pMP, idx1) (LocalMapping.cc:892), and the
 *     member reads exactly that, pKF1->GetMapPoint(idx1), once per idx1 (ORBmatcher.cc:1049-1055);
 *   - vbMatched2 is declared and never set (ORBmatcher.cc:1027, :1083), so the searches of different idx1 do not see one another;
 *   - neighbour j's own map points change only in iteration j (LocalMapping.cc:893), after its search;
 *   - both call sites construct the matcher with checkOri = false (LocalMapping.cc:500, Tracking.cc:4236): no rotation histogram
 *     couples the keypoints.  That is why there is no checkOri argument here: with it the rule below would not hold.
 * Hence the sequential result for neighbour j = row j computed from the state at loop entry, with matches12[j][idx1] set to -1 for
 * every idx1 that received a map point in the iterations before j.  The caller applies the mask while it walks the rows:
 * `if (mpCurrentKeyFrame->GetMapPoint(idx1)) continue;` in front of each pair (tests/test_gpu_triangulation_neighbours.py replays
 * the sequential loop against this rule).
 *
 * Pinhole form: R1w / t1w / Cw1 / cam1 of kf1 as in orbm_search_for_triangulation; R2w [K][9], t2w [K][3], cam2 [K][4] per neighbour.
 * KannalaBrandt8 form: n_left1 and cams1 ([1][8] or [2][8]) of kf1; per neighbour n_left2 [K], ep [K][2], cams2 [K][2][8] and
 * T12 [K][4][12] - the strides are those of a rig also for keyframes without a second camera, which use [j][0] only.
 * ORBX_E_ARG, with orbm_last_error naming the neighbour ("neighbour <j>: ..."), for:
 *   - whatever the per-pair entry refuses, per neighbour that is not skipped (KannalaBrandt8 form: a rig paired with a single-camera
 *     keyframe included); both forms check every neighbour as orbm_search_for_triangulation_kb8 does - NULL arrays, nlevels, octaves
 *     outside [0, nlevels), node_start decreasing, node members outside [0, n), a node of more than 65535 members - because the
 *     kernels read the scale tables from device memory;
 *   - K < 0, a NULL table with K > 0 (a table only the searched neighbours need may be NULL when all are skipped);
 *   - more than 2^31 - 1 keypoint pairs in shared nodes, summed over the neighbours. */
int orbm_search_for_triangulation_neighbours(orbm_t *m, const orbm_keyframe_t *kf1, int K, const orbm_keyframe_t *kf2 /*[K]*/,
                                             const float *R1w, const float *t1w, const float *Cw1, const float *cam1,
                                             const float *R2w /*[K][9]*/, const float *t2w /*[K][3]*/, const float *cam2 /*[K][4]*/,
                                             const uint8_t *skip /*[K] or NULL*/, int bOnlyStereo, int bCoarse,
                                             int32_t *matches12 /*[K][kf1->n]*/, int32_t *nmatches /*[K]*/);
int orbm_search_for_triangulation_kb8_neighbours(orbm_t *m, const orbm_keyframe_t *kf1, int n_left1, int K,
                                                 const orbm_keyframe_t *kf2 /*[K]*/, const int32_t *n_left2 /*[K]*/,
                                                 const float *ep /*[K][2]*/, const float *cams1, const float *cams2 /*[K][2][8]*/,
                                                 const float *T12 /*[K][4][12]*/, const uint8_t *skip, int bOnlyStereo, int bCoarse,
                                                 int32_t *matches12, int32_t *nmatches);

/* ---- LocalMapping::CreateNewMapPoints (LocalMapping.cc:470-905): the searches above AND the geometric body of the loop ----
 * The body of the loop over the matched pairs (:605-880: rays and parallax, cv::SVD triangulation or KeyFrame::UnprojectStereo, two
 * depth tests, two chi-square reprojection tests, the far-point and scale-consistency tests) is stated once for host and device
 * (csrc/orb_ref_newpoints.h) and returns one of the codes below; every `continue` of :605-880 has its own value. */
enum {
  ORBM_NP_NO_MATCH = 0,        /* matches12[j][idx1] < 0: the pair does not exist */
  ORBM_NP_ACCEPTED = 1,        /* :883 reached */
  ORBM_NP_LOW_PARALLAX = 2,    /* :782  no stereo and very low parallax */
  ORBM_NP_ZERO_W = 3,          /* :763  the homogeneous coordinate of vt.row(3) is 0 */
  ORBM_NP_EMPTY_STEREO = 4,    /* :788  UnprojectStereo returned the empty matrix (mvDepth <= 0) */
  ORBM_NP_BEHIND1 = 5,         /* :793  z1 <= 0 */
  ORBM_NP_BEHIND2 = 6,         /* :797  z2 <= 0 */
  ORBM_NP_REPROJ1 = 7,         /* :814  monocular reprojection error in the new keyframe */
  ORBM_NP_REPROJ1_STEREO = 8,  /* :827  stereo reprojection error in the new keyframe */
  ORBM_NP_REPROJ2 = 9,         /* :842  monocular reprojection error in the neighbour */
  ORBM_NP_REPROJ2_STEREO = 10, /* :853  stereo reprojection error in the neighbour */
  ORBM_NP_ZERO_DIST = 11,      /* :866  dist1 == 0 || dist2 == 0 */
  ORBM_NP_FAR = 12,            /* :869  mbFarPoints and a distance >= mThFarPoints */
  ORBM_NP_SCALE = 13,          /* :879  ratioDist against ratioOctave */
  ORBM_NP_NSTATUS = 14
};

/* One new map point: MapPoint(x3D, mpCurrentKeyFrame, map) observed by keypoint idx1 of the new keyframe and idx2 of kf2[neighbour] */
typedef struct { int32_t neighbour, idx1, idx2; float x3D[3]; } orbm_new_point_t;

/* What the body reads of a keyframe beyond orbm_keyframe_t (host pointers).  Poses are 12 floats with row stride 4. */
typedef struct {
  const float *Tcw;        /* [Rcw | tcw] = GetRotation() | GetTranslation() = rows 0..2 of GetPose() */
  const float *Ow;         /* GetCameraCenter() [3] */
  const float *Tcw_right;  /* rigs: rows 0..2 of GetRightPose(); NULL otherwise */
  const float *Ow_right;   /* rigs: GetRightCameraCenter() [3]; NULL otherwise */
  const float *Twc;        /* rows 0..2 of Twc (UnprojectStereo); may be NULL when no keypoint has u_right >= 0 */
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  const float *depth;      /* mvDepth [n]; may be NULL when no keypoint has u_right >= 0 */
  const orbx_keypoint_t *keys;   /* mvKeys [n] (UnprojectStereo reads mvKeys, not mvKeysUn); NULL as for depth */
} orbm_keyframe_geometry_t;

/* The body alone, over arrays of pairs, for inspection and tests.  The keyframe's constants by value and one record per keypoint:
 *   cam[0] / cam[1] = mvParameters of mpCamera / mpCamera2 ({fx, fy, cx, cy} Pinhole, {fx, fy, cx, cy, k0..k3} KannalaBrandt8);
 *   Tcw[1] / Ow[1] the right camera's of a rig; n_left = NLeft (-1: no second camera, then bStereo = u_right >= 0);
 *   sf / sigma2 = mvScaleFactors / mvLevelSigma2; an octave is taken modulo ORBX_MAX_LEVELS.
 *   obs: x, y, octave of the keypoint the reference picks (:613-626: mvKeysUn, or mvKeys / mvKeysRight of a rig), u_right = mvuRight,
 *   depth = mvDepth, key_x / key_y = mvKeys[idx].pt, right = idx >= NLeft of a rig. */
typedef struct {
  float Tcw[2][12], Ow[2][3], Twc[12], cam[2][8];
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  float sf[ORBX_MAX_LEVELS], sigma2[ORBX_MAX_LEVELS];
  int32_t cam_type;   /* 0 Pinhole, 1 KannalaBrandt8 */
  int32_t n_left;
} orbm_new_point_camera_t;
typedef struct { float x, y; int32_t octave; float u_right, depth, key_x, key_y; int32_t right; } orbm_new_point_obs_t;

/* status[i] = ORBM_NP_* of pair i of (c1, c2): obs1[i] of the new keyframe, obs2[i] of the neighbour; x3D [n][3] is written where the
 * status is ORBM_NP_ACCEPTED.  scale_factor1 = mpCurrentKeyFrame->mfScaleFactor (ratioFactor = 1.5f * it, :521), far_points /
 * th_far_points = mbFarPoints / mThFarPoints.  No GPU call; the device form takes device arrays for obs / status / x3D (c1, c2 stay
 * host structs) and is asynchronous on `stream`.  0, ORBX_E_ARG (a NULL pointer, n < 0, cam_type outside {0, 1}) or ORBX_E_HIP. */
int orbm_new_point_geometry(int n, const orbm_new_point_camera_t *c1, const orbm_new_point_camera_t *c2, const orbm_new_point_obs_t *obs1,
                            const orbm_new_point_obs_t *obs2, float scale_factor1, int far_points, float th_far_points, uint8_t *status,
                            float *x3D);
int orbm_new_point_geometry_device(int n, const orbm_new_point_camera_t *c1, const orbm_new_point_camera_t *c2,
                                   const orbm_new_point_obs_t *d_obs1, const orbm_new_point_obs_t *d_obs2, float scale_factor1,
                                   int far_points, float th_far_points, uint8_t *d_status, float *d_x3D, void *stream);

/* New keyframe plus neighbours in, the list of new map points out: the one-call searches above (bOnlyStereo = 0 as at the call site,
 * LocalMapping.cc:583), then the body on every matched pair ON THE DEVICE, reading the rows the search just wrote there; one upload,
 * one synchronisation, and a download of the list (plus what the caller asks for).
 *
 * The SEQUENTIAL RULE, next to the MASKING RULE above.  The reference's loop creates a point for (j, idx1) exactly when
 *   (a) the body accepts the pair (idx1, matches12[j][idx1]) of the row computed from the state at loop entry, and
 *   (b) no neighbour j' < j that is not skipped has an accepted pair for the same idx1.
 * Argument:
 *   - a keypoint idx1 of the new keyframe is masked only by mpCurrentKeyFrame->AddMapPoint(pMP, idx1) (LocalMapping.cc:892);
 *   - that line is reached only when the body accepted the pair (every test in front of it ends in `continue`);
 *   - row j (MASKING RULE) and the geometry of a pair depend on nothing else the loop changes: the poses, cameras, keypoints, depths
 *     and scale tables of both keyframes are read-only in the loop, and pKF2->AddMapPoint (:893) touches neighbour j after its search;
 *   - so idx1 is free in iteration j exactly when no earlier iteration accepted it, and then the loop sees the loop-entry pair.
 * Hence the list = { (j, idx1) : status[j][idx1] == ORBM_NP_ACCEPTED and j is the smallest such neighbour of idx1 }, in the loop's
 * creation order: j ascending, idx1 ascending (vMatchedIndices is ascending in idx1).  An idx1 appears at most once.
 * Consequence: when CheckNewKeyFrames() ends the loop in front of neighbour i (LocalMapping.cc:528), the caller keeps the entries
 * with neighbour < i - a prefix of the list, and exactly what the shortened loop would have created, because (b) looks at smaller j only.
 *
 * Arguments: those of the search entry of the same form (bOnlyStereo fixed to 0), then g1 / g2 [K] and scale_factor1 =
 * mpCurrentKeyFrame->mfScaleFactor, far_points / th_far_points.  Pinhole form: mono and rectified-stereo keypoints mix per keypoint;
 * cam1 / cam2[j] are also the parameters of pCamera1 / pCamera2.  KannalaBrandt8 form: cams1 / cams2[j] likewise; for rigs g->Tcw_right
 * and g->Ow_right are read and u_right / depth / keys are not.
 * Out: points [cap] in creation order, the count is returned; a list longer than cap returns the needed count and writes no point
 * (an idx1 appears once, so cap = kf1->n always suffices).  Optional (NULL: not downloaded): status [K][kf1->n] = ORBM_NP_* of the
 * loop-entry pair, NOT masked by (b); matches12 [K][kf1->n] and nmatches [K] as in the search entry (nmatches needs matches12).
 * skip, K == 0, kf1->n == 0: as in the search entries - an empty list (status 0, rows -1), the device untouched.
 * ORBX_E_ARG, orbm_last_error naming the neighbour where there is one, for whatever the search entry refuses, and for
 *   - a NULL g1, g2 (K > 0 and a neighbour searched), points with cap > 0, cap < 0, nmatches without matches12;
 *   - a NULL Tcw or Ow, for rigs a NULL Tcw_right or Ow_right ("neighbour <j>: NULL pose");
 *   - a NULL depth, keys or Twc of a keyframe that has a keypoint with u_right >= 0 ("neighbour <j>: NULL mvDepth, mvKeys or Twc"). */
int orbm_create_new_map_points(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_geometry_t *g1, float scale_factor1, int K,
                               const orbm_keyframe_t *kf2 /*[K]*/, const orbm_keyframe_geometry_t *g2 /*[K]*/, const float *R1w,
                               const float *t1w, const float *Cw1, const float *cam1, const float *R2w /*[K][9]*/,
                               const float *t2w /*[K][3]*/, const float *cam2 /*[K][4]*/, const uint8_t *skip /*[K] or NULL*/, int bCoarse,
                               int far_points, float th_far_points, orbm_new_point_t *points, int cap, uint8_t *status /*[K][kf1->n] or NULL*/,
                               int32_t *matches12 /*[K][kf1->n] or NULL*/, int32_t *nmatches /*[K] or NULL*/);
int orbm_create_new_map_points_kb8(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_geometry_t *g1, float scale_factor1,
                                   int n_left1, int K, const orbm_keyframe_t *kf2 /*[K]*/, const orbm_keyframe_geometry_t *g2 /*[K]*/,
                                   const int32_t *n_left2 /*[K]*/, const float *ep /*[K][2]*/, const float *cams1,
                                   const float *cams2 /*[K][2][8]*/, const float *T12 /*[K][4][12]*/, const uint8_t *skip, int bCoarse,
                                   int far_points, float th_far_points, orbm_new_point_t *points, int cap, uint8_t *status,
                                   int32_t *matches12, int32_t *nmatches);

/* int ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched,
 *                                         vector<int> &vnMatches12, int windowSize)              (ORBmatcher.cc:722-837)
 * f1 / f2: mvKeysUn + mDescriptors of the two frames (f2 with its image bounds; u_right unused); prev_matched[2*n1]
 * (in/out) = vbPrevMatched; matches12[n1] (out) = vnMatches12.  nnratio / checkOri = mfNNratio / mbCheckOrientation.
 * Only level-0 keypoints of F1 take part (:737-739) and, through the level window, only level-0 keypoints of F2.
 * The per-query window search + Hamming runs in the projection-search scan kernel, the sequential
 * vMatchedDistance rule (:762, :788) in one wavefront on the device; the steal bookkeeping (:781-785), the rotation
 * histogram and the vbPrevMatched update are replayed on the host.  Returns nmatches. */
int orbm_search_for_initialization(orbm_t *m, const orbm_frame_t *f1, const orbm_frame_t *f2, float *prev_matched,
                                   int window_size, float nnratio, int checkOri, int32_t *matches12);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches)   (ORBmatcher.cc:273-469,
 * Frame::Nleft == -1).  kf: the keyframe (has_mappoint[i] = pMP && !pMP->isBad(), keys_un = mvKeysUn for the angle);
 * f: the frame in the same flattened form (keys_un = F.mvKeys, descriptors = F.mDescriptors, node_* = F.mFeatVec;
 * u_right / has_mappoint / scale tables unused).  matchF[f->n] (out) = index of the keyframe keypoint whose map point
 * the frame keypoint received (vpMapPointMatches[i] = vpMapPointsKF[matchF[i]]) or -1.  One wavefront per shared
 * vocabulary node on the device; rotation histogram on the host.  Returns nmatches. */
int orbm_search_by_bow(orbm_t *m, const orbm_keyframe_t *kf, const orbm_keyframe_t *f, float nnratio, int checkOri, int32_t *matchF);

/* The same member for a fisheye-stereo frame (Frame::Nleft != -1, ORBmatcher.cc:338-363, :405-436): f holds mvKeys followed by
 * mvKeysRight / the concatenated mDescriptors, keypoints >= n_left_f are the right image's; kf->keys_un likewise carries the
 * keypoint the reference picks for the angle (:391-394).  A keyframe keypoint can hand its map point to one left AND one right
 * frame keypoint; matchF marks both. */
int orbm_search_by_bow_fisheye(orbm_t *m, const orbm_keyframe_t *kf, const orbm_keyframe_t *f, int n_left_f, float nnratio, int checkOri,
                               int32_t *matchF);

/* int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12)    (ORBmatcher.cc:839-979)
 * has_mappoint[i] = pMP && !pMP->isBad() on both sides; matches12[kf1->n] (out) = keypoint of kf2 whose map point
 * keypoint i of kf1 was matched with (vpMatches12[i] = vpMapPoints2[matches12[i]]) or -1.  Returns nmatches. */
int orbm_search_by_bow_keyframes(orbm_t *m, const orbm_keyframe_t *kf1, const orbm_keyframe_t *kf2, float nnratio, int checkOri,
                                 int32_t *matches12);

/* SearchByBoW of ONE frame or keyframe against ALL candidates in one call: the two loops of the reference that call the members
 * above once per candidate -
 *   Tracking::Relocalization (Tracking.cc:3796-3816): matcher.SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]) per
 *     relocalisation candidate, for every frame while tracking is lost;
 *   LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:724-739): matcherBoW.SearchByBoW(mpCurrentKF, vpCovKFi[j],
 *     vvpMatchedMPs[j]) for a candidate and its best covisibles, per loop and merge candidate.
 * The fixed operand is staged once, every searched candidate's descriptors, flags and feature-vector members go up in the same block
 * with a record table and the flat list of (candidate, shared node) items: one upload, one fill of the rows with -1 on the device, one
 * launch over every item (one wavefront each; the node's first 64 second-operand keypoints are held in registers across the walk, the
 * walked keypoint comes through the scalar path), one launch that does the rotation histogram per candidate on the device, one download
 * of the rows and the K counts, one synchronisation.
 *
 * Row j of matchF [K][f->n] is bit for bit what orbm_search_by_bow returns for (kf[j], f) with the same nnratio and checkOri - with
 * n_left_f >= 0 what orbm_search_by_bow_fisheye returns - and nmatches[j] that call's return value.  Row j of matches12 [K][kf1->n] is
 * bit for bit what orbm_search_by_bow_keyframes returns for (kf1, kf2[j]), rotation-histogram pruning included.
 * skip[j] != 0 (skip may be NULL) stands for the reference's isBad() `continue` (Tracking.cc:3799-3800, LoopClosing.cc:726-727):
 * row j is all -1, nmatches[j] = 0, and candidate j is neither validated nor uploaded.
 * Returns the sum of nmatches.  K == 0, every candidate skipped, an empty fixed operand, no pair that shares a node: 0 without touching
 * the device, the rows still written as all -1.
 *
 * Why the searches may leave the two loops - the INDEPENDENCE RULE:
 *   - each call writes only its own vpMapPointMatches / vpMatches12, which the member itself starts as all-NULL (ORBmatcher.cc:277,
 *     ORBmatcher.cc:852) and which is the only result it reads back;
 *   - beyond that the member reads the operands' map-point tables, descriptors and feature vectors, and no statement of
 *     Tracking.cc:3796-3816 or LoopClosing.cc:724-739 changes any of them: the bodies only test nmatches, set up a solver, or collect
 *     the matched points;
 *   - the isBad() tests inside the member (ORBmatcher.cc:310, :865-870, :896-903) are a snapshot at the call, exactly as the
 *     has_mappoint arrays of the per-pair entries are;
 *   - hence row j is the per-pair result from the state at loop entry, with no mask and no replay (unlike the MASKING RULE above,
 *     nothing between the iterations feeds the next search).
 *
 * ORBX_E_HIP, or ORBX_E_ARG with orbm_last_error naming the candidate ("candidate <j>: ...") where there is one, for:
 *   - whatever the per-pair entry refuses, per searched candidate: n < 0, a NULL array of a pair in which both sides have keypoints and
 *     nodes, a shared node of the second operand with more than 2048 members;
 *   - a node_start that is negative or decreases, a node_idx outside [0, n) in a shared node (the kernels index device memory with them);
 *   - K < 0, a NULL table with K > 0, n_left_f outside [-1, f->n], more than 2^31 - 1 items.
 * Every candidate is validated before the first device call: nothing is launched and no output is written when an argument is refused. */

/* Tracking::Relocalization, Tracking.cc:3796-3816: K candidate keyframes against ONE frame */
int orbm_search_by_bow_candidates(orbm_t *m, int K, const orbm_keyframe_t *kf /*[K]*/, const orbm_keyframe_t *f,
                                  int n_left_f /* -1: Frame::Nleft == -1 */, const uint8_t *skip /*[K] or NULL*/,
                                  float nnratio, int checkOri, int32_t *matchF /*[K][f->n]*/, int32_t *nmatches /*[K]*/);

/* LoopClosing::DetectCommonRegionsFromBoW, LoopClosing.cc:724-739: ONE keyframe against K keyframes */
int orbm_search_by_bow_keyframes_candidates(orbm_t *m, const orbm_keyframe_t *kf1, int K, const orbm_keyframe_t *kf2 /*[K]*/,
                                            const uint8_t *skip /*[K] or NULL*/, float nnratio, int checkOri,
                                            int32_t *matches12 /*[K][kf1->n]*/, int32_t *nmatches /*[K]*/);

/* void MapPoint::ComputeDistinctiveDescriptors()  (MapPoint.cc:350-436), batched over map points: the descriptors that
 * observe map point p are desc[32*start[p] .. 32*start[p+1]) in the order the reference collects them (observations map
 * order, left index before right index); best[p] (out) = BestIdx within that group (-1 for an empty group), i.e.
 * mDescriptor = vDescriptors[best[p]].  At most 1024 observations per map point.  Returns 0. */
int orbm_distinctive_descriptors(orbm_t *m, int nmp, const int32_t *start, const uint8_t *desc, int32_t *best);

/* void MapPoint::ComputeDistinctiveDescriptors()  (MapPoint.cc:350-436) AND void MapPoint::UpdateNormalAndDepth()  (MapPoint.cc:467-547)
 * for ALL map points of one call: the loop of LocalMapping.cc:1040-1053 (every map point of the current keyframe), the same pair after
 * LocalMapping::CreateNewMapPoints (LocalMapping.cc:890-897) and at initialisation and map creation (Tracking.cc:2353, :2374, :2552,
 * :3400, :4460).  One upload block, one launch (k_update_map_points: one wavefront per map point; for up to 64 entries every descriptor
 * is loaded once into its lane's registers and row i reaches the lanes by a lane read), one download, one synchronisation.
 *
 * best[p] (out) = the entry index RELATIVE to start[p] of the descriptor MapPoint.cc:389-435 keeps (mDescriptor = that entry's row): the
 * first least median (vDists[0.5*(N'-1)], strict `<`) over the N' entries with in_desc set, or -1 where no entry has in_desc set (the
 * reference returns without writing, :389).  normal[p], min_dist[p], max_dist[p] (out) = mNormalVector, mfMinDistance, mfMaxDistance of
 * :543-545, from EVERY entry (the walk of :489-511 has no isBad() test); the arithmetic is csrc/orb_ref_mappoint.h, host and device.
 * A point without entries (observations.empty(), :365 / :483) gets best[p] = -1 and its three float outputs are LEFT UNTOUCHED, as both
 * members return without writing.  A point lying in one of its camera centres gives NaN, as the reference's arithmetic does.
 *
 * Why the points may leave the loop - INDEPENDENCE:
 *   - a call of either member reads the keyframes' descriptors and camera centres, the point's own mWorldPos, its own mObservations and
 *     its own mpRefKF (with that keyframe's scale table), and writes only the point's own mDescriptor, mNormalVector, mfMinDistance and
 *     mfMaxDistance;
 *   - none of what is read is written by either member, so no call changes an input of the call for another point, and the order of the
 *     points does not matter;
 *   - a point listed twice is recomputed from the same inputs to the same values;
 *   - isBad() of a keyframe or of the point, and a concurrent change of the observations or the position by another thread, are a
 *     snapshot at the member's own lock in the reference; a caller that batches takes the snapshot earlier and must compare it again
 *     when it writes (csrc/adapter/snippets/MapPoint_UpdateBatch_hip.cc does).
 *
 * ORBX_E_ARG before anything is uploaded or launched, with no output written, for: a NULL handle, struct or output; nmp < 0; a NULL array
 * that is indexed; start[0] != 0 or a start that decreases; more than 1024 entries of one point.  nmp == 0 returns 0. */
typedef struct {
  int32_t nmp;
  const int32_t *start;       /* [nmp+1], entries of point p are start[p] .. start[p+1]-1: one entry per (keyframe, camera) that
                                 observes it, in the order of the reference's walk (:371-386, :489-511) */
  const uint8_t *desc;        /* [nobs][32] pKF->mDescriptors.row(index) */
  const float   *centre;      /* [nobs][3]  GetCameraCenter() or GetRightCameraCenter() of that entry */
  const uint8_t *in_desc;     /* [nobs]     1 = !pKF->isBad() (:375): the entry takes part in the descriptor choice; the normal
                                 takes every entry (:489-511 has no such test) */
  const float   *pos;         /* [nmp][3]   mWorldPos */
  const float   *ref_centre;  /* [nmp][3]   pRefKF->GetCameraCenter() */
  const float   *ref_scale;   /* [nmp]      pRefKF->mvScaleFactors[level], level by :522-531 */
  const float   *ref_max_scale; /* [nmp]    pRefKF->mvScaleFactors[nLevels-1] */
} orbm_map_point_update_t;

int orbm_update_map_points(orbm_t *m, const orbm_map_point_update_t *u,
                           int32_t *best /*[nmp]*/, float *normal /*[nmp][3]*/, float *min_dist /*[nmp]*/, float *max_dist /*[nmp]*/);
/* MapPoint.cc:486-545 for ONE map point on the host, no handle: the same functions of csrc/orb_ref_mappoint.h, hence the same bits.
 * n == 0 returns 0 and writes nothing; ORBX_E_ARG for n < 0 or a NULL pointer. */
int orbm_map_point_normal_depth(int n, const float *centre /*[n][3]*/, const float *pos, const float *ref_centre,
                                float ref_scale, float ref_max_scale, float *normal, float *min_dist, float *max_dist);

/* void LocalMapping::KeyFrameCulling()  (LocalMapping.cc:1158-1310): the redundancy counts of every local keyframe and the cull loop,
 * on the device.  The loop body is LocalMapping.cc:1204-1266; what a culled keyframe changes is KeyFrame::SetBadFlag's walk over its
 * map points (KeyFrame.cc:670-677) through MapPoint::EraseObservation (MapPoint.cc:168-202) and MapPoint::SetBadFlag
 * (MapPoint.cc:217-226).  Every compare is a function of csrc/orb_ref_culling.h, host and device; parity with the literal model of
 * tests/keyframe_culling_model.py is exact.
 *
 * A ROW is one keypoint i of one local keyframe k; an ENTRY is one element of a map point's mObservations.
 *   - Row i of keyframe k is dead when row_point[i] < 0 (no map point, :1211) or bad[p] (:1213) and, when mono == 0, when
 *     row_depth[i] > th_depth[k] || row_depth[i] < 0 in float (:1217).  Otherwise it counts in nMPs (:1221).
 *   - When n_obs[p] > 3 (:1222) the row is redundant when more than 3 live entries of p have obs_kf != k (:1232) and
 *     obs_level <= row_level[i] + 1 (:1250).  The break at the fourth hit (:1253) changes no result.
 *   - Keyframe k passes when nRedundantObservations > redundant_th * nMPs as C evaluates it (:1266): a float product with nMPs
 *     converted to float, compared in float with the left side converted.  It is not a double product.
 *   - Erasing keyframe c visits every row of c with row_point >= 0 in row order (KeyFrame.cc:670-677).  Where point p has a live entry
 *     with obs_kf == c, n_obs[p] -= obs_w[entry] (MapPoint.cc:179-187) and the entry dies (:189); n_obs[p] <= 2 (:195) turns the point
 *     bad and all its entries die (MapPoint.cc:223-225).  A second row of c with the same point (a rig's left and right index) finds no
 *     entry and does nothing.  The entries of a point that is bad on entry are dead: a bad point's mObservations is empty.
 *
 * SEQUENTIAL CULLING RULE - why the loop may run on the device, and why the stepwise walk equals the sequential loop:
 *   - the loop body for keyframe k reads, of mutable state, only isBad(), Observations() and GetObservations() of k's map points, and
 *     k's own isBad(); it writes, through SetBadFlag of k, exactly these three of k's map points (and k's isBad()).  No other state that
 *     the body reads is written by the loop: levels, depths, mThDepth and the keyframe list are fixed at loop entry;
 *   - validity only shrinks: an entry never comes back to life, n_obs never rises, a bad point never recovers.  So a row's status at
 *     keyframe k's turn is its loop-entry status unless an erase touched the row's point before k's turn, and re-evaluating the rows of
 *     touched points from the current state gives what the reference computes at that turn;
 *   - an erase is applied once per point although the rows are handled in parallel: the keyframe's entry of a point is claimed by one
 *     atomic compare-and-swap, and the order of the points within one erase does not matter because an erase of c changes only
 *     per-point state and reads no other point;
 *   - the stepwise form stops at each passing keyframe and applies its erase, or not, at the start of the next step, before any later
 *     keyframe is evaluated: exactly the reference's order of SetBadFlag and the next iteration.  Keyframes that do not pass change
 *     nothing, so walking over them inside one step equals visiting them one at a time.
 *
 * ORBX_E_ARG with a message, nothing launched and no output written, for: a NULL handle (device forms), struct or output; a NULL array
 * that is indexed (row_depth only when mono == 0; erasable, n_obs_out and bad_out may be NULL); K, P or a count < 0; K above
 * ORBM_CULL_MAX_KEYFRAMES; row_start[0] / obs_start[0] not 0 or a start table that decreases; more rows in one keyframe than
 * ORBM_MAX_KEYPOINTS; a row_point outside [-1, P); an obs_kf outside [-1, K); an obs_w outside {1, 2}; two entries of one point with
 * the same obs_kf >= 0 (mObservations is a map); a NaN redundant_th; step without open.  K == 0 returns 0 without touching the device.
 * There is no cap on the entries of one point: lists above 64 entries are walked by a wavefront in 64-entry tiles. */
#define ORBM_CULL_MAX_KEYFRAMES 1024   /* the reference's loop stops after 101 (:1305) */
typedef struct {
  int32_t K;                  /* local keyframes in the loop's order (GetVectorCovisibleKeyFrames, :1166) */
  const uint8_t *skip;        /* [K] mnId == GetInitKFid() || isBad()  (:1200): no counts, never culled */
  const float   *th_depth;    /* [K] pKF->mThDepth (:1217) */
  const int32_t *row_start;   /* [K+1] rows of keyframe k = its keypoints i (:1208), row_start[k] .. row_start[k+1]-1 */
  const int32_t *row_point;   /* [R] index into the point table, -1 = no map point (:1211) */
  const int32_t *row_level;   /* [R] scaleLevel of :1224-1226 */
  const float   *row_depth;   /* [R] pKF->mvDepth[i] (:1217); may be NULL when mono != 0 */
  int32_t P;                  /* distinct map points */
  const uint8_t *bad;         /* [P] pMP->isBad() (:1213) */
  const int32_t *n_obs;       /* [P] pMP->Observations() (:1222) */
  const int32_t *obs_start;   /* [P+1] entries of point p = obs_start[p] .. obs_start[p+1]-1 (GetObservations, :1227) */
  const int32_t *obs_kf;      /* [E] index into the K keyframes, -1 = an observer that is not in the list */
  const int32_t *obs_level;   /* [E] scaleLeveli of :1236-1248 */
  const uint8_t *obs_w;       /* [E] what EraseObservation subtracts for this keyframe: 1 or 2 (MapPoint.cc:179-187) */
  int32_t mono;               /* mbMonocular (:1215) */
  float redundant_th;         /* :1168-1174 */
} orbm_culling_t;

/* The whole loop under the non-inertial rule (:1300-1303): keyframe k is culled when it passes, !skip[k] and erasable[k] (NULL = all 1);
 * erasable[k] stands for !mbNotErase, and where it is 0 SetBadFlag returns without erasing (KeyFrame.cc:650-655).  n_mps[k], n_red[k] =
 * nMPs and nRedundantObservations at keyframe k's turn, culled[k] = 1 where it was erased; skipped keyframes get 0, 0, 0.
 * n_obs_out[p], bad_out[p] (either may be NULL) = Observations() and isBad() after the loop.  One upload, k_cull_count, k_cull_walk,
 * one download, one synchronisation.  The `count > 100` and mbAbortBA breaks (:1305) are the caller's: pass the keyframes that the
 * loop would reach.  Returns 0. */
int orbm_keyframe_culling(orbm_t *m, const orbm_culling_t *c, const uint8_t *erasable /*[K] or NULL*/, int32_t *n_mps /*[K]*/,
                          int32_t *n_red /*[K]*/, uint8_t *culled /*[K]*/, int32_t *n_obs_out /*[P] or NULL*/, uint8_t *bad_out /*[P] or NULL*/);
/* The stepwise form, for the inertial branch (:1268-1299), where the live objects decide, and for callers that cannot read mbNotErase.
 * open uploads the tables into buffers of the handle that no other entry uses and computes the loop-entry status of every row; it
 * discards an unfinished walk.  Every step first erases the keyframe that the previous step returned if applied != 0, then walks on
 * to the next unskipped keyframe that passes, writes n_mps[j] / n_red[j] of every keyframe j it walked (0, 0 for a skipped one; other
 * elements are left alone) and returns that keyframe's index in *k, or K at the end (further steps return K again).  Other orbm_*
 * calls between steps are allowed.  One launch, one download and one synchronisation per step. */
int orbm_keyframe_culling_open(orbm_t *m, const orbm_culling_t *c);
int orbm_keyframe_culling_step(orbm_t *m, int applied, int32_t *k, int32_t *n_mps /*[K]*/, int32_t *n_red /*[K]*/);
/* The one-call form on the CPU with the functions of csrc/orb_ref_culling.h, one object at a time in the loop's order: no handle, same
 * outputs, same refusals (the message: orbm_keyframe_culling_host_error).  It exists so that the statement can be tested without a
 * device; it is not a fallback of the device forms. */
int orbm_keyframe_culling_host(const orbm_culling_t *c, const uint8_t *erasable, int32_t *n_mps, int32_t *n_red, uint8_t *culled,
                               int32_t *n_obs_out, uint8_t *bad_out);
const char *orbm_keyframe_culling_host_error(void);

/* ---- void Tracking::UpdateLocalMap()  (Tracking.cc:3542-3553) = UpdateLocalKeyFrames (:3590-3762) + UpdateLocalPoints (:3559-3587),
 * and the counter and ordered lists of void KeyFrame::UpdateConnections(bool)  (KeyFrame.cc:407-492) ----
 * Both members are one vote: every row's map point gives one increment to each keyframe that observes it.  Every compare is a function
 * of csrc/orb_ref_localmap.h, host and device; all results are integers.  Parity: exact against the literal model of
 * tests/update_local_map_model.py; Tracking.cc and KeyFrame.cc are not compiled under oracle/_ref, so the reference text itself is unpinned.
 *
 * The tables, a flattened view of the map that both members read.  The plain entries take host pointers; the _device entry takes the
 * same struct holding device pointers: the caller keeps the tables resident and rewrites what local mapping changed with copies of its
 * own.  The library keeps no store.
 *
 * RANK RULE - next to the MASKING, SEQUENTIAL, INDEPENDENCE, FUSE, SEARCH-AND-FUSE, ORDER and SEQUENTIAL CULLING RULES above.  The
 * reference iterates map<KeyFrame*,int> and set<KeyFrame*> and sorts pair<int,KeyFrame*>, so its results depend on pointer values, but
 * only on their ORDER.  kf_rank[g] are distinct integers that order the keyframes as their addresses do, and that is all either member
 * reads of them:
 *   - iteration of keyframeCounter / KFcounter (Tracking.cc:3658, KeyFrame.cc:455): ascending rank, so kf_max is the lowest-ranked
 *     keyframe among those with the largest count (the compare is a strict >);
 *   - iteration of spChilds (Tracking.cc:3708): kf_child lists every keyframe's children in ascending rank;
 *   - the ties of sort(vPairs) (KeyFrame.cc:477): (weight, pointer) ascending, reversed by push_front (:480-484), which gives
 *     descending weight and, among equal weights, descending rank.
 * Rank is apart from the slot g so that a new keyframe costs a rewrite of one array of G ints and no re-index of the observations.
 *
 * STAMP NOTE.  The reference marks keyframes and points with mnTrackReferenceForFrame = mCurrentFrame.mnId, and nothing but
 * Tracking.cc:3577-3750 writes that member.  A fresh set of marks per call is therefore the same thing for every frame id that has not
 * been through UpdateLocalMap before; id 0, the member's initial value, never reaches TrackLocalMap.  The adapter snippet still writes
 * the stamps back on the live objects.
 *
 * CONNECTIONS RULE.  KFcounter of a keyframe reads mvpMapPoints, the observations, isBad() and GetMap(); UpdateConnections of any
 * keyframe writes none of them (it writes mConnectedKeyFrameWeights, the two ordered vectors, mpParent / mspChildrens and, through
 * AddConnection, the same of other keyframes).  So the rows of T targets may be counted from the state at loop entry, in one call.
 * What the member WRITES stays the caller's, replayed in the loop's order: the target's own three tables, AddConnection on the others
 * with the UpdateBestCovisibles re-sort it triggers (KeyFrame.cc:205-242), and mpParent / AddChild at the first connection (:501-527). */
#define ORBM_MAP_MAX_KEYFRAMES 16384      /* G: what one workgroup sorts in LDS (csrc/orb_sort.h) */
#define ORBM_MAP_BEST 10                  /* GetBestCovisibilityKeyFrames(10) (Tracking.cc:3690) */
typedef struct {
  int32_t G;                      /* keyframes; g is a stable slot, not an order */
  const int32_t *kf_rank;         /* [G] distinct: the RANK RULE */
  const uint8_t *kf_bad;          /* [G] KeyFrame::isBad() (Tracking.cc:3662, :3696, :3711; KeyFrame.cc:434) */
  const int32_t *kf_map;          /* [G] an integer standing for GetMap() (KeyFrame.cc:434) */
  const int32_t *kf_row_start;    /* [G+1] rows of keyframe g = its mvpMapPoints (Tracking.cc:3569, KeyFrame.cc:415), at most ORBM_MAX_KEYPOINTS */
  const int32_t *row_point;       /* [R] index into the points, -1 = NULL */
  const int32_t *kf_best;         /* [G][10] GetBestCovisibilityKeyFrames(10) in its order, padded with -1 (KeyFrame.cc:259-266) */
  const int32_t *kf_child_start;  /* [G+1] */
  const int32_t *kf_child;        /* GetChilds() in the set's iteration order (Tracking.cc:3707-3708) */
  const int32_t *kf_parent;       /* [G] GetParent() or -1 (Tracking.cc:3723) */
  const int32_t *kf_prev;         /* [G] mPrevKF or -1 (Tracking.cc:3751); may be NULL when inertial == 0 */
  int32_t P;                      /* map points */
  const uint8_t *pt_bad;          /* [P] MapPoint::isBad() */
  const int32_t *obs_start;       /* [P+1] */
  const int32_t *obs_kf;          /* [E] GetObservations(): one entry per observing keyframe, as slots; the entries of a bad point are not read */
} orbm_map_graph_t;

/* UpdateLocalMap for one frame.  frame_point[N] = mCurrentFrame.mvpMapPoints (or mLastFrame's, Tracking.cc:3596-3646) as point indices,
 * -1 = NULL.  inertial = the sensor test of :3737, last_kf = mCurrentFrame.mpLastKeyFrame or -1.
 *   - the vote (:3599-3646): every slot with a point that is not bad gives one vote per entry of the point, with no filter on the voted
 *     keyframe; a point in two slots votes twice; slot_bad[s] = 1 where the reference sets the slot to NULL (the point is bad), else 0;
 *   - the first list (:3649-3675): the voted keyframes in rank order without the bad ones; kf_max / max_votes = pKFmax and max (-1 / 0
 *     when there is none: mpReferenceKF stays);
 *   - the expansion (:3680-3733) over the first list only: at the top of a trip stop when the list holds more than 80 (so it can end at
 *     81, 82 or 83); the first of kf_best that is not bad and not marked; the first child that is not bad and not marked; the parent if
 *     there is one and it is not marked, WITHOUT an isBad test, and its break leaves the OUTER loop (:3724-3731);
 *   - the temporal tail (:3737-3754) when inertial and the list is below 80: from last_kf, up to 20 trips, stop at -1; an unmarked
 *     keyframe is appended and the walk steps to kf_prev; at a marked one the reference does not advance, so nothing more changes;
 *   - local points (:3559-3587): the local keyframes in REVERSE list order, each one's rows in row order; NULL rows, marked points and
 *     bad points are skipped, the rest appended and marked.
 * local_kf [cap_kf] / *n_local_kf = mvpLocalKeyFrames, local_point [cap_pts] / *n_local_point = mvpLocalMapPoints.  One staged upload,
 * k_covis_vote, k_local_kf_walk, k_lp_first, k_lp_count, k_lp_write, one download, one synchronisation.  Returns 0; ORBX_E_CAP when a
 * list does not fit (the counts hold what is needed, the lists are not written).  N == 0 returns 0 without touching the device, with
 * both counts 0, kf_max -1 and max_votes 0.
 *
 * ORBX_E_ARG with a message, nothing launched and no output written, for: a NULL handle (device forms), struct or output; a NULL
 * array that is indexed (kf_prev only when inertial; kf_child, row_point and obs_kf only when they have elements); G, P, N, T or a
 * capacity < 0; G above ORBM_MAP_MAX_KEYFRAMES; a start table that does not begin at 0 or that decreases; more rows in one keyframe
 * than ORBM_MAX_KEYPOINTS; a row_point or frame_point outside [-1, P); an obs_kf, kf_child or target outside [0, G); a kf_best,
 * kf_parent, kf_prev or last_kf outside [-1, G); duplicate ranks; two entries of one point with the same keyframe; a target listed
 * twice; inertial with kf_prev == NULL. */
int orbm_update_local_map(orbm_t *m, const orbm_map_graph_t *graph, int N, const int32_t *frame_point, int inertial, int last_kf,
                          int cap_kf, int cap_pts, int32_t *local_kf, int32_t *n_local_kf, int32_t *kf_max, int32_t *max_votes,
                          uint8_t *slot_bad /*[N]*/, int32_t *local_point, int32_t *n_local_point);
/* The same with everything resident: *graph is a HOST struct holding DEVICE pointers, frame_point and every output are device arrays,
 * the counts are device ints.  Asynchronous on `stream`, nothing touches the host.  Writes are clamped at the capacities and the
 * counts report what was needed.  The tables cannot be looked at: only the scalars are checked (NULL pointers, G, P, N, capacities,
 * last_kf); an index outside its table is the caller's error, though a point or keyframe index that is out of range is skipped where
 * it is read.  The handle's scratch (counters, the per-point word, the whole keyframe list) is shared by the calls on one handle:
 * they must follow each other on one stream.  The per-point word is cleared by a memset at the start of every call.  N == 0 launches
 * nothing and writes nothing. */
int orbm_update_local_map_device(orbm_t *m, const orbm_map_graph_t *d_graph, int N, const int32_t *d_frame_point, int inertial, int last_kf,
                                 int cap_kf, int cap_pts, int32_t *d_local_kf, int32_t *d_n_local_kf, int32_t *d_kf_max,
                                 int32_t *d_max_votes, uint8_t *d_slot_bad, int32_t *d_local_point, int32_t *d_n_local_point, void *stream);
/* The CPU statement from the same header, one object at a time in the reference's order: no handle, same outputs, same refusals (the
 * message: orbm_update_local_map_host_error, which serves orbm_update_connections_host too).  Not a fallback of the device forms. */
int orbm_update_local_map_host(const orbm_map_graph_t *graph, int N, const int32_t *frame_point, int inertial, int last_kf, int cap_kf,
                               int cap_pts, int32_t *local_kf, int32_t *n_local_kf, int32_t *kf_max, int32_t *max_votes,
                               uint8_t *slot_bad, int32_t *local_point, int32_t *n_local_point);
const char *orbm_update_local_map_host_error(void);

/* KFcounter and the ordered lists of KeyFrame::UpdateConnections for the T keyframes targets[T], all counted from the state at entry
 * (CONNECTIONS RULE).  For target t (KeyFrame.cc:409-484): every row with a point that is not bad gives one count to every entry k of
 * the point unless k == t, kf_bad[k] or kf_map[k] != kf_map[t] (:434).  A rig point held in two rows of t counts twice; from the other
 * side it counts by the other keyframe's rows, so the weights need not be symmetric.  An empty counter (:442) means the member returns
 * having written nothing: n_conn = 0, kf_max -1, nmax 0.  Otherwise, in rank order: kf_max / nmax by a strict > (:459), the pairs
 * with count >= th (:464; th = 15 in the reference), or if there are none the single pair (nmax, kf_max) (:471-475), sorted as the
 * RANK RULE says.  Outputs: conn_kf / conn_w [conn_start[t] .. conn_start[t+1]) = mConnectedKeyFrameWeights in rank order;
 * ord_kf / ord_w [ord_start[t] .. ord_start[t+1]) = mvpOrderedConnectedKeyFrames / mvOrderedWeights; kf_max[t], nmax[t].  cap = the
 * elements of each of the four list arrays.  One staged upload, k_covis_vote, k_conn_walk, k_conn_pack, one download, one
 * synchronisation.  Returns 0; ORBX_E_CAP when conn_start[T] exceeds cap (the start tables, kf_max and nmax are written, the lists
 * are not); T == 0 returns 0 without touching the device; refusals as above.
 * COST: the device block of one call holds the counters and four work strips at stride G per target, 20 * T * G bytes beside the
 * tables (1.5 MB at T = 150, G = 500; 21 MB at T = 65, G = 16 384; about 5.4 GB at T = G = 16 384, which fails as that allocation
 * would, with ORBX_E_HIP).  A loop over many keyframes of a large map is passed in chunks of targets; the chunks are independent
 * (CONNECTIONS RULE). */
int orbm_update_connections(orbm_t *m, const orbm_map_graph_t *graph, int T, const int32_t *targets, int th, int cap,
                            int32_t *conn_start /*[T+1]*/, int32_t *conn_kf, int32_t *conn_w, int32_t *ord_start /*[T+1]*/,
                            int32_t *ord_kf, int32_t *ord_w, int32_t *kf_max /*[T]*/, int32_t *nmax /*[T]*/);
int orbm_update_connections_host(const orbm_map_graph_t *graph, int T, const int32_t *targets, int th, int cap, int32_t *conn_start,
                                 int32_t *conn_kf, int32_t *conn_w, int32_t *ord_start, int32_t *ord_kf, int32_t *ord_w,
                                 int32_t *kf_max, int32_t *nmax);

/* The arrays of an orbm_local_map_t from the local-point list that orbm_update_local_map_device left on the device and caller-resident
 * per-point tables (all device pointers, indexed by point: d_Xw / d_normal 3 floats, d_max_dist / d_min_dist, d_mpdesc 32 bytes at a
 * 4-byte aligned address, d_obs or NULL = all 1).  Element i < min(*d_n_local_point, cap) of every array of *out (a HOST struct of
 * device pointers, written although the type says const; obs may be NULL, Tcw and n are not touched) is the point d_local_point[i];
 * eligible = !pt_bad && the point is in no slot of d_frame_point[N] (Tracking.cc:3453-3471, :3483-3487); *d_map_n = that count, which
 * is what orbm_search_local_points_batch_device takes as d_map_n with npairs = 1.  Asynchronous on `stream`, nothing touches the host;
 * uses the handle's scratch as orbm_update_local_map_device does.  ORBX_E_ARG for a NULL required pointer, P, N or cap < 0. */
int orbm_gather_local_map_device(orbm_t *m, int P, int N, const int32_t *d_frame_point, const int32_t *d_local_point,
                                 const int32_t *d_n_local_point, int cap, const uint8_t *d_pt_bad, const float *d_Xw, const float *d_normal,
                                 const float *d_max_dist, const float *d_min_dist, const uint8_t *d_mpdesc, const uint8_t *d_obs,
                                 const orbm_local_map_t *out, int32_t *d_map_n, void *stream);

/* ---- bool TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated) ----
 * (TwoViewReconstruction.cc:39-127; what GeometricCamera::ReconstructWithTwoViews calls for both camera models, Pinhole.cpp:126-133,
 * KannalaBrandt8.cpp:211-234, from Tracking::MonocularInitialization, Tracking.cc:2492).  Every expression of the member and of what it
 * calls (Normalize, ComputeH21 / ComputeF21 with cv::SVD, CheckHomography / CheckFundamental, ReconstructH / ReconstructF, DecomposeE,
 * CheckRT, Triangulate) is stated once for host and device in csrc/orb_ref_twoview.h.
 *
 * The TWO-VIEW RULE: why the iterations may leave the two loops of FindHomography / FindFundamental (:153-176, :204-227).
 *   - The minimal sets are drawn before either loop starts (:77-96) and neither loop changes them.
 *   - An iteration reads nothing an earlier iteration wrote except the running best (score, and with it H21 / F21 and the inlier vector):
 *     vPn1i / vPn2i, H21i / H12i / F21i, vbCurrentInliers and currentScore are all overwritten from the set alone (:156-168, :207-219);
 *     the keypoints, the matches and the normalisation are read-only.
 *   - The running best is a strict maximum taken in order (`currentScore > score` from score = 0, :170, :221): the loop keeps the FIRST
 *     iteration whose score is the greatest one above 0, and none when no score is above 0 (a NaN score compares false and never wins).
 * Hence the 2 x iterations hypotheses and scores are computed independently, and the winner per model is the smallest iteration that
 * attains the maximum of the scores above 0.  Within one score the additions keep the reference's order (match ascending, the first
 * image's term before the second's, into one float), and CheckRT's loop writes disjoint entries per match except the sorted list of
 * cosParallax values, of which only the value at one rank is read (:902-905): equal values are interchangeable.
 *
 * Device form: Normalize on the host in front of the upload (it walks every keypoint of both frames, which arrive from the host), then
 * k_tv_hypotheses, k_tv_score, k_tv_winner, one synchronisation, the 3 x 3 algebra of ReconstructH / ReconstructF and the decisions on the
 * host (compares and one acos per hypothesis), k_tv_check_rt and k_tv_cos_rank, a second synchronisation.
 *
 * keys1 [n1] / keys2 [n2]: vKeys1 / vKeys2 (mvKeysUn of the two frames, the form orbm_search_for_initialization's frames use);
 * matches12 [n1]: vMatches12, exactly what orbm_search_for_initialization returns (< 0: no match); N = the number of entries >= 0.
 * K [9]: mK, row-major; sigma, iterations: the constructor's (1.0, 200 at Tracking.cc:2431 / the camera models).
 * sets [iterations][8]: mvSets, indices into the N matches in ascending first-keypoint order.  They come from the CALLER: the reference
 * draws them with DUtils::Random::RandomInt over libc rand(), seeded once per process (Random.cpp:38-50), later calls continue the
 * stream; only the caller can reproduce that, and the library never calls rand().
 * Out: returns 1 / 0 = the member's bool; on 1 R21 [9], t21 [3], vP3D [n1][3] (zeros where not triangulated) and vbTriangulated [n1];
 * on 0 they are left alone (the reference leaves its arguments alone or empties R21 / t21).
 * details (NULL, or a struct whose non-NULL members are filled as far as the call got; the rest of an array is zeros):
 *   SH, SF [1]; best_it [2] the winning iteration of H, F or -1; H21, F21 [9] (zeros when the model is absent); inliersH, inliersF [N];
 *   score [2][iterations]; used_H [1]: 1 ReconstructH ran, 0 ReconstructF, -1 neither (SH + SF == 0); nhyp [1]: 0, 4 or 8 hypotheses checked
 *   (0: ReconstructH returned at :601); R [8][9], t [8][3], nGood [8], parallax [8] per hypothesis in the reference's order;
 *   chosen [1] or -1; status [8][N] = ORBM_TV_* of every (hypothesis, match).
 * ORBX_E_ARG, named by orbm_last_error, nothing launched, for: a NULL handle or required pointer; n1 or n2 < 0; fewer than 8 matches (the
 * reference's draw runs off its vector there); iterations < 1; a set index outside [0, N); a match index >= n2.
 * Undefined in the reference and unspecified here: a NaN cosParallax among the accepted ones (std::sort on it). */
enum {
  ORBM_TV_NOT_INLIER = 0,    /* :836  !vbMatchesInliers[i] */
  ORBM_TV_GOOD = 1,          /* :897  accepted, cosParallax < 0.99998: vbGood */
  ORBM_TV_LOW_PARALLAX = 2,  /* :894  accepted and counted, not vbGood */
  ORBM_TV_NONFINITE = 3,     /* :848  a non-finite coordinate of p3dC1 */
  ORBM_TV_BEHIND1 = 4,       /* :862  depth in the first camera */
  ORBM_TV_BEHIND2 = 5,       /* :868  depth in the second camera */
  ORBM_TV_REPROJ1 = 6,       /* :879  reprojection error in the first image */
  ORBM_TV_REPROJ2 = 7,       /* :890  reprojection error in the second image */
  ORBM_TV_NSTATUS = 8
};
typedef struct {
  float *SH, *SF;
  int32_t *best_it;
  float *H21, *F21;
  uint8_t *inliersH, *inliersF;
  float *score;
  int32_t *used_H, *nhyp;
  float *R, *t;
  int32_t *nGood;
  float *parallax;
  int32_t *chosen;
  uint8_t *status;
} orbm_two_view_details_t;
int orbm_two_view_reconstruct(orbm_t *m, const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2,
                              const int32_t *matches12 /*[n1]*/, const float *K /*[9]*/, float sigma, int iterations,
                              const int32_t *sets /*[iterations][8]*/, float *R21, float *t21, float *vP3D, uint8_t *vbTriangulated,
                              const orbm_two_view_details_t *details);
/* The same result on the CPU from csrc/orb_ref_twoview.h, without a device or a handle (the message of a refusal:
 * orbm_two_view_host_error).  For tests without a GPU; it is not a fallback of the device form. */
int orbm_two_view_reconstruct_host(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                   const float *K, float sigma, int iterations, const int32_t *sets, float *R21, float *t21, float *vP3D,
                                   uint8_t *vbTriangulated, const orbm_two_view_details_t *details);
const char *orbm_two_view_host_error(void);
/* The two device stages alone, each with its CPU form (same refusals as above where the arguments exist).
 * Models: H21, H12, F21 [iterations][9] of every iteration (H12 = H21i.inv()), score [2][iterations], best_it [2], masks [2][N] (the
 * winners' inlier vectors, zeros for an absent model).  Every output is required. */
int orbm_two_view_models(orbm_t *m, const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                         float sigma, int iterations, const int32_t *sets, float *H21, float *H12, float *F21, float *score,
                         int32_t *best_it, uint8_t *masks);
int orbm_two_view_models_host(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                              float sigma, int iterations, const int32_t *sets, float *H21, float *H12, float *F21, float *score,
                              int32_t *best_it, uint8_t *masks);
/* CheckRT (:802-911) for nhyp in [1, 8] caller-supplied hypotheses R [nhyp][9], t [nhyp][3] and an inlier vector inliers [N]:
 * vP3D [nhyp][n1][3] and vbGood [nhyp][n1] (zeros elsewhere), status [nhyp][N], nGood [nhyp], cos_rank [nhyp] =
 * vCosParallax[min(50, nGood - 1)] of the sorted vector (0 when nGood == 0), parallax [nhyp] (degrees; acos on the host).  Every output
 * is required; at least one match (not eight) is. */
int orbm_two_view_check_rt(orbm_t *m, const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                           const uint8_t *inliers, const float *K, float sigma, int nhyp, const float *R, const float *t, float *vP3D,
                           uint8_t *vbGood, uint8_t *status, int32_t *nGood, float *cos_rank, float *parallax);
int orbm_two_view_check_rt_host(const orbx_keypoint_t *keys1, int n1, const orbx_keypoint_t *keys2, int n2, const int32_t *matches12,
                                const uint8_t *inliers, const float *K, float sigma, int nhyp, const float *R, const float *t, float *vP3D,
                                uint8_t *vbGood, uint8_t *status, int32_t *nGood, float *cos_rank, float *parallax);

/* ---- Sim3Solver: the constructor, SetRansacParameters, ComputeSim3, CheckInliers and one call of iterate ----
 * (Sim3Solver.cc:35-530; built at LoopClosing.cc:810-824 from the matches of SearchByBoW against a candidate and its covisibles, the
 * step between orbm_search_by_bow_keyframes_candidates and the Sim3 SearchByProjection.)  Every expression is stated once for host and
 * device in csrc/orb_ref_sim3.h.
 *
 * The SIM3 RULE: why the iterations may leave the loop of iterate (:194-237, :267-315).
 *   - The set of iteration i is drawn from mvAllIndices alone (:199-213); nothing an iteration computes reaches a later draw.
 *   - ComputeSim3 and CheckInliers overwrite mR12i, mt12i, ms12i, mT12i, mT21i, mvbInliersi and mnInliersi from the set alone; the camera
 *     coordinates, the projections and the thresholds are read-only behind the constructor.
 *   - The only state carried across iterations, and across calls of iterate, is the running best, taken with `>=` (:219, :292): of equal
 *     counts the LATER iteration wins.
 *   - An iteration ends the loop where its count is >= the best before it AND > mRansacMinInliers, strictly (:228, :301): a count equal
 *     to mRansacMinInliers does not converge.
 * Hence all counts are computed independently, and one ordered pass over them gives the stop iteration, the best hypothesis, bNoMore
 * (mnIterations >= mRansacMaxIts, :239, :317) and, for the five-argument overload, whether this call improved the best (its bestSim3).
 *
 * Device form: the constructor's two transforms and projections on the host in front of one staged upload (they walk host data);
 * k_sim3_hypotheses (centroids, M, N, OpenCV's float Jacobi eigen per iteration); a first synchronisation; per hypothesis on the host
 * the double-libm tail (atan2, cv::Rodrigues, scale, translation, T12, T21: no device sin / cos / atan2 for double is pinned against
 * glibc); k_sim3_check for every (iteration, pair); k_sim3_winner, the ordered pass and the winner's mask; one download, the second
 * synchronisation.
 *
 * The problem: n1 = mN1 (the length of vpMatched12) and the N pairs the constructor keeps (:85-137), in its order:
 *   idx1 [N] mvnIndices1 (ascending, in [0, n1)); Xw1 / Xw2 [N][3] the world positions of pMP1 / pMP2; sigma2_1 / sigma2_2 [N]
 *   pKF1->mvLevelSigma2[kp1.octave] / pKFm->mvLevelSigma2[kp2.octave] (pKFm: the keyframe the pair was matched in, :101-115);
 *   Tcw1 / Tcw2 [16] row-major poses of pKF1 / pKF2 - pKF2's even for a pair matched in another keyframe (:132);
 *   cam_type1/2 (0 Pinhole, 1 KannalaBrandt8) and cam_params1/2 (4 / 8 floats) of pKF1->mpCamera / pKF2->mpCamera;
 *   fix_scale mbFixScale; min_inliers mRansacMinInliers; iterations_done / max_iterations: mnIterations at entry and mRansacMaxIts
 *   (orbm_sim3_ransac_iterations).
 * sets [iterations][3]: the pairs of every iteration of this call, indices into the N pairs after the reference's swap-with-last draw
 * (:204-212), so distinct within a set.  They come from the CALLER (DUtils::Random over libc rand()); the library never calls rand().
 * The loop runs min(iterations, max_iterations - iterations_done) iterations at the most; later sets are not part of the answer.
 * best_inliers_in: mnBestInliers at entry.
 * The result: converged (bConverge / a non-empty return of the four-argument overload), it_stop (iterations consumed, what mnIterations
 * grows by), best_it (the iteration of this call that holds the best, -1 when none reached best_inliers_in), best_inliers (mnBestInliers
 * at exit), improved (1 when best_it >= 0), no_more (bNoMore); T12 [16], R12 [9], t12 [3], s12 of best_it (mBestT12, mBestRotation,
 * mBestTranslation, mBestScale; zeros when best_it < 0: the members keep their values); best_mask [N] mvbBestInliers of best_it (zeros
 * when best_it < 0) and vbInliers [n1], spread through idx1 on convergence and zeros otherwise - the caller's two buffers, both required.
 * details (NULL, or a struct whose non-NULL members are filled): counts [iterations], T12 / T21 [iterations][16], quat [iterations][4]
 * (evec.row(0)), masks [iterations][N] - of EVERY iteration of the call, also those behind it_stop; wall_ms [4], the host's clock over
 * the device form's four phases, for measurements (tools/sim3_solver_bench.py; zeros from the CPU form): the constructor's host loop;
 * staging, upload, k_sim3_hypotheses and its download up to the first synchronisation; the host tail; the transforms' upload,
 * k_sim3_check, k_sim3_winner and the download up to the second synchronisation.
 * N < min_inliers is the reference's bNoMore return (:182, :252): converged = 0, it_stop = 0, no_more = 1, nothing launched.
 * ORBX_E_ARG, named by orbm_last_error, nothing launched, for: NULL where required; N < 3 (the draw runs off its vector); N > n1; an idx1
 * outside [0, n1) or not ascending; a set index outside [0, N) or repeated within a set; iterations < 1; min_inliers < 0;
 * iterations_done < 0; an unknown camera type; a sigma2 that is negative, not finite or >= 9e15 (its size_t conversion is undefined). */
typedef struct {
  int32_t n1, N;
  const int32_t *idx1;
  const float *Xw1, *Xw2;
  const float *sigma2_1, *sigma2_2;
  const float *Tcw1, *Tcw2;
  int32_t cam_type1, cam_type2;
  const float *cam_params1, *cam_params2;
  int32_t fix_scale, min_inliers;
  int32_t iterations_done, max_iterations;
} orbm_sim3_problem_t;
typedef struct {
  int32_t converged, it_stop, best_it, best_inliers, improved, no_more;
  float T12[16], R12[9], t12[3], s12;
  uint8_t *best_mask; /* [N], the caller's */
  uint8_t *vbInliers; /* [n1], the caller's */
} orbm_sim3_result_t;
typedef struct {
  int32_t *counts;
  float *T12, *T21, *quat;
  uint8_t *masks;
  double *wall_ms;
} orbm_sim3_details_t;
int orbm_sim3_solve(orbm_t *m, const orbm_sim3_problem_t *problem, int iterations, const int32_t *sets /*[iterations][3]*/,
                    int best_inliers_in, orbm_sim3_result_t *result, const orbm_sim3_details_t *details);
/* The same result on the CPU from csrc/orb_ref_sim3.h, without a device or a handle (the message of a refusal: orbm_sim3_host_error).
 * For tests without a GPU; it is not a fallback of the device form. */
int orbm_sim3_solve_host(const orbm_sim3_problem_t *problem, int iterations, const int32_t *sets, int best_inliers_in,
                         orbm_sim3_result_t *result, const orbm_sim3_details_t *details);
const char *orbm_sim3_host_error(void);
/* The stages alone, each with its CPU form (the same refusals where the arguments exist; every output is required).
 * Hypotheses: ComputeSim3 for every set: T12, T21 [iterations][16], quat [iterations][4].  (k_sim3_hypotheses and the host tail.) */
int orbm_sim3_hypotheses(orbm_t *m, const orbm_sim3_problem_t *problem, int iterations, const int32_t *sets, float *T12, float *T21,
                         float *quat);
int orbm_sim3_hypotheses_host(const orbm_sim3_problem_t *problem, int iterations, const int32_t *sets, float *T12, float *T21, float *quat);
/* Check: CheckInliers for nhyp >= 1 caller-supplied transforms T12, T21 [nhyp][16]: counts [nhyp], masks [nhyp][N].  (k_sim3_check.) */
int orbm_sim3_check(orbm_t *m, const orbm_sim3_problem_t *problem, int nhyp, const float *T12, const float *T21, int32_t *counts,
                    uint8_t *masks);
int orbm_sim3_check_host(const orbm_sim3_problem_t *problem, int nhyp, const float *T12, const float *T21, int32_t *counts, uint8_t *masks);
/* SetRansacParameters (:150-174): the value it leaves in mRansacMaxIts for N kept pairs.  epsilon as float, pow, log and ceil in double,
 * min_inliers == N gives 1, then max(1, min(nIterations, max_its)). */
int orbm_sim3_ransac_iterations(double probability, int min_inliers, int max_its, int N);

/* cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, matches, 2) as called by Frame::ComputeStereoFishEyeMatches
 * (Frame.cc:1246): idx2[2i..], dist2[2i..] = train index and distance of the nearest and second nearest train descriptor
 * of query i (-1 where nc < 2).  Equal distances are ordered by train index; the only consumer (the ratio test of
 * Frame.cc:1252) gives the same result for any tie order.  Host pointers.  Returns 0. */
int orbm_knn_match2(orbm_t *m, const uint8_t *q, int nq, const uint8_t *c, int nc, int32_t *idx2, int32_t *dist2);

/* Brute-force Hamming (K8): dist[i*nc + j] = popcount(q_i xor c_j); host pointers. */
int orbm_hamming_matrix(orbm_t *m, const uint8_t *q, int nq, const uint8_t *c, int nc, uint16_t *dist);

/* ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2416-2458) on bin sizes; host. */
void orbm_three_maxima(const int *histo_sizes, int L, int *ind1, int *ind2, int *ind3);
/* ORBmatcher::RadiusByViewingCos (ORBmatcher.cc:216-222). */
float orbm_radius_by_viewing_cos(float viewCos);
/* GeometricCamera::project(cv::Point3f): type 0 Pinhole (Pinhole.cpp:46-49), 1 KannalaBrandt8
 * (KannalaBrandt8.cpp:29-45); params = mvParameters. */
void orbm_project(int cam_type, const float *params, float X, float Y, float Z, float *u, float *v);

/* Frame::UndistortKeyPoints (Frame.cc:837-870) and Frame::ComputeImageBounds (:872-899): the step between extract and
 * match.  cv::undistortPoints(pts, K, D, R = I, P = K) is an fp64 fixed-point iteration on <= N points, so it
 * stays on the host.  K = {fx, fy, cx, cy}; D = {k1, k2, p1, p2[, k3]} (nD = 4 or 5).
 * D[0] == 0 copies the keypoints unchanged (Frame.cc:839-843) and gives the bounds [0,cols] x [0,rows].
 * keys_un may alias keys (only pt is rewritten). */
void orbm_undistort_keypoints(int n, const orbx_keypoint_t *keys, const float *K, const float *D, int nD, orbx_keypoint_t *keys_un);
void orbm_image_bounds(int cols, int rows, const float *K, const float *D, int nD, float *min_x, float *max_x, float *min_y,
                       float *max_y);
/* Frame::UndistortKeyPoints (Frame.cc:837-870) for `nframes` frames whose keypoints are resident in HBM (the output of
 * orbx_extract_batch_device): frame f's keypoints at d_keys + f * key_stride, its count at d_counts[f * count_stride]
 * (d_counts == NULL: n_const keypoints per frame).  Same arithmetic, same bits as orbm_undistort_keypoints (one source,
 * undistort_point in csrc/orb_ref_geometry.h).  d_keys_un may alias d_keys.  Asynchronous on `stream`; returns 0 or an ORBX_E_* code. */
int orbm_undistort_keypoints_batch_device(orbm_t *m, const orbx_keypoint_t *d_keys, int key_stride, const int32_t *d_counts,
                                          int count_stride, int n_const, int nframes, const float *K, const float *D, int nD,
                                          orbx_keypoint_t *d_keys_un, void *stream);

/* How the projection searches enumerate a query's candidates.  The reference walks the grid cells of the query's window
 * (Frame::GetFeaturesInArea, Frame.cc:744-813); on the device that is k_match_walk, right for tracking-sized windows, while
 * k_match_scan streams every keypoint of the frame past every query, right when the windows cover the frame (BASELINE's
 * 1000x1000 setting, relocalisation).  ORBM_SCAN_AUTO (default) decides per frame pair on the device: the walk when no
 * query's window exceeds 256 grid cells and the frame has at most 2048 keypoints, else the scan.  The two produce the same
 * candidate lists, so results never depend on the mode; it exists for tests and measurements (the environment variable
 * ORBM_SCAN_MODE=0|1|2 sets a new handle's initial mode: measured cost of the per-pair vote on the 1000x1000 workload 0.5 %).
 * Returns 0 or ORBX_E_ARG. */
#define ORBM_SCAN_AUTO 0
#define ORBM_SCAN_DENSE 1
#define ORBM_SCAN_WALK 2
int orbm_set_scan_mode(orbm_t *m, int mode);
/* Where open-window searches (window = whole grid, no level filter: BASELINE's 1000 x 1000 setting, relocalisation-style
 * searches) compute their Hamming distances (ORBmatcher::DescriptorDistance, ORBmatcher.cc:2463-2483):
 *   0  xor + popcount on the vector ALU (k_match_scan) like every other query block;
 *   1  open-window query blocks as exact int8 dot products on the matrix pipe (k_match_scan_mfma: monocular frames of at most
 *      2048 keypoints, batch launches);
 *   2  (default) as 1, and frame pairs ALL of whose queries are open build their candidate lists inside k_match_resolve (fused
 *      form): per 64-query chunk, at the chunk's turn, with every keypoint a committed claim holds masked out, so that the lists
 *      are not exhausted by earlier chunks' claims (ORBmatcher.cc:89-91, :124-130 resolved without the refresh passes).
 * Engines 1 and 2 also put the two brute-force entries on the matrix pipe: orbm_hamming_matrix (k_hamming_matrix_mfma) and
 * orbm_knn_match2 (k_knn2_mfma, train sets below 2^20 descriptors); engine 0 keeps their vector-ALU kernels.
 * Results do not depend on it; the tests run all three. */
int orbm_set_hamming_engine(orbm_t *m, int engine);

/* Time of the last search kernel launch sequence (HIP events on its stream), ms; <0 if profiling is off. */
void orbm_set_profiling(orbm_t *m, int enable);
float orbm_get_last_ms(orbm_t *m);
/* Per-kernel split, averaged over the searches launched since orbm_set_profiling(m, 1) (ring of 32 event sets, as for
 * orbx_get_stage_ms): ms[0] = k_match_walk + k_match_scan (+ k_topk_merge), ms[1] = k_match_resolve.  Returns 2, or 0 if unavailable. */
int orbm_get_stage_ms(orbm_t *m, float *ms, int cap);

/* ------------------------------------------------------------------------------------------------------------------
 * ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>): the transform behind Frame::ComputeBoW
 * (Frame.cc:828-835) and KeyFrame::ComputeBoW (KeyFrame.cc:100-110), both
 *     mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1194 over the descent of :1217-1259, BowVector.cpp:34-84,
 * FeatureVector.cpp:31-45).  It produces the DBoW2::FeatureVector that orbm_keyframe_t carries into SearchByBoW,
 * SearchForTriangulation and CreateNewMapPoints.  The arithmetic is stated once, in csrc/orb_ref_voc.h, for the host form and
 * the kernels (csrc/orb_voc_kernels.h).  L2_NORM scoring (type 1) is refused; so is a levelsup for which the vocabulary has a
 * childless node of weight > 0 above level L - levelsup (the reference leaves the NodeId of a feature that ends there unset, :1251,
 * and files the feature under it, :1160).  A childless node of weight <= 0 up there only stops features and is accepted.
 * ------------------------------------------------------------------------------------------------------------------ */

/* m_nodes flattened in id order; node 0 is the root (it is not in the text file, TemplatedVocabulary.h:1376-1377).
 * The children of a node are rebuilt in ascending node id, which is the loader's push_back order (:1385-1392); word ids are
 * counted over the nodes with is_leaf set, in id order (:1408-1415; is_leaf[0] is not read).  The child count of a node is
 * whatever parent[] says and is NOT bounded by k: every trailing empty line of the text file makes one more node (:1378-1386)
 * whose parent is an indeterminate read (`>> pid` fails and stores nothing, :1389-1392; seen with g++ -O2: the previous
 * line's parent, flagged as a leaf, weight 0), so a node of a loaded k-ary vocabulary can own more than k children.  The
 * descent ends at a node without children (Node::isLeaf() is children.empty(), :328), flagged or not; an unflagged one
 * answers word 0 (Node(), :316) with its own weight. */
typedef struct {
  int32_t k, L;                /* m_k, m_L (L gives the level of the FeatureVector's nodes, :1226) */
  int32_t weighting;           /* m_weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY (BowVector.h:39-45) */
  int32_t scoring;             /* m_scoring: 0 L1_NORM, 1 L2_NORM (refused), 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA,
                                  5 DOT_PRODUCT (BowVector.h:48-56); decides the normalisation, ScoringObject.h:74-89 */
  int32_t n_nodes;             /* m_nodes.size() >= 1 */
  const uint32_t *parent;      /* [n_nodes] Node::parent; parent[i] < i for i >= 1 (parent[0] is not read) */
  const uint8_t *is_leaf;      /* [n_nodes] the node owns a word: m_words[node.word_id] == &node */
  const uint8_t *descriptor;   /* [n_nodes][32] Node::descriptor */
  const double *weight;        /* [n_nodes] Node::weight */
} orbv_nodes_t;

typedef struct orbv_handle orbv_t;

/* Copies the tables, re-laid so that the children of a node are contiguous.  device >= 0 also uploads them; device = -1 gives
 * a handle WITHOUT device tables, on which only orbv_transform_host works and the device entries return ORBX_E_ARG: it
 * exists so that the statement can be tested where there is no GPU, and is not a fallback.  NULL on failure (a NULL table,
 * n_nodes < 1, parent[i] >= i, weighting / scoring out of range, L2_NORM scoring, a HIP error), with the reason in
 * orbv_last_error(NULL). */
orbv_t *orbv_create(const orbv_nodes_t *nodes, int device);
void orbv_destroy(orbv_t *v);
/* The reason of the CALLING THREAD's last failed orbv_* call (Tracking and LocalMapping share one vocabulary, so the text is
 * kept per thread, not per handle); v may be NULL. */
const char *orbv_last_error(const orbv_t *v);
/* m_nodes.size(), m_words.size(), the largest child count, the level (root = 0) of the shallowest childless node of weight > 0
 * (INT32_MAX without one). */
int orbv_n_nodes(const orbv_t *v);
int orbv_n_words(const orbv_t *v);
int orbv_max_children(const orbv_t *v);
int orbv_min_leaf_level(const orbv_t *v);

/* transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1126-1194) for descriptors[n][32], host pointers.
 *   word_of_feature[n], node_of_feature[n]  (optional) WordId and NodeId of every feature, stopped ones included (:1217-1259); 0 as
 *                                           the NodeId of a stopped feature that ended above level L - levelsup
 *   bow_id[n], bow_val[n], *n_bow           DBoW2::BowVector in key order: the first *n_bow entries are written
 *   fv_node_id[n], fv_start[n + 1], fv_idx[n], *n_fv
 *                                           DBoW2::FeatureVector exactly as orbm_keyframe_t reads it (node_id, node_start,
 *                                           node_idx, n_nodes): the first *n_fv, *n_fv + 1 and fv_start[*n_fv] entries
 * A feature whose word has weight > 0 enters both containers, a feature on a stop word neither (:1157, :1185).  n == 0 and a
 * vocabulary without words (:1134) give empty containers (*n_bow = *n_fv = 0, fv_start[0] = 0).
 * orbv_transform_host is csrc/orb_ref_voc.h in plain C++ over the handle's host tables with two std::maps.  orbv_transform is
 * one upload, k_voc_descend and k_voc_collect, one download, one synchronisation; it may be called on one handle from several
 * host threads at once (each call takes a stream and a workspace from the handle's pool).
 * Both validate everything before anything is written or launched.  ORBX_E_ARG: a NULL handle or required pointer, n < 0 or
 * above ORBM_MAX_KEYPOINTS, a levelsup the vocabulary's shape refuses (orbv_last_error names the node), orbv_transform on a
 * device = -1 handle.  Returns 0, ORBX_E_ARG or ORBX_E_HIP. */
int orbv_transform_host(const orbv_t *v, const uint8_t *descriptors, int n, int levelsup, uint32_t *word_of_feature,
                        uint32_t *node_of_feature, uint32_t *bow_id, double *bow_val, int32_t *n_bow, uint32_t *fv_node_id,
                        int32_t *fv_start, int32_t *fv_idx, int32_t *n_fv);
int orbv_transform(orbv_t *v, const uint8_t *descriptors, int n, int levelsup, uint32_t *word_of_feature,
                   uint32_t *node_of_feature, uint32_t *bow_id, double *bow_val, int32_t *n_bow, uint32_t *fv_node_id,
                   int32_t *fv_start, int32_t *fv_idx, int32_t *n_fv);

/* The same transform (TemplatedVocabulary.h:1126-1194) for `nframes` frames resident in HBM, asynchronous on `stream`: the same
 * two kernels with a grid over all frames.  d_descriptors[nframes][cap][32] (16-byte aligned); frame p has
 * min(max(d_n[p * n_stride], 0), cap) live descriptors, so the extractor's d_counts plugs in with n_stride = 2.  Frame p's
 * outputs start at p * cap (d_fv_start at p * (cap + 1)) in the per-frame layout above; d_n_bow[nframes], d_n_fv[nframes];
 * d_word / d_node [nframes][cap] are optional.  d_scratch: orbv_batch_scratch_bytes(nframes, cap) bytes of device memory that
 * belong to the call until the stream has passed it (no state of the handle is written, so calls may overlap).
 * ORBX_E_ARG: as orbv_transform, nframes outside [0, 65535], cap outside [1, ORBM_MAX_KEYPOINTS], n_stride <= 0, a
 * misaligned d_descriptors / d_bow_val.  nframes == 0 launches nothing.
 * orbv_transform_batch_device_form is the same call with the descent kernel chosen: 0 = k_voc_descend (a 16-lane row per
 * descriptor, what every other entry runs), 1 = k_voc_descend_lane (a lane per descriptor); results do not depend on it, it
 * exists for tests and for tools/bow_transform_bench.py. */
size_t orbv_batch_scratch_bytes(int nframes, int cap);
int orbv_transform_batch_device(orbv_t *v, const uint8_t *d_descriptors, int nframes, int cap, const int32_t *d_n, int n_stride,
                                int levelsup, uint32_t *d_word, uint32_t *d_node, uint32_t *d_bow_id, double *d_bow_val,
                                int32_t *d_n_bow, uint32_t *d_fv_node_id, int32_t *d_fv_start, int32_t *d_fv_idx, int32_t *d_n_fv,
                                void *d_scratch, void *stream);
int orbv_transform_batch_device_form(orbv_t *v, int descend_form, const uint8_t *d_descriptors, int nframes, int cap,
                                     const int32_t *d_n, int n_stride, int levelsup, uint32_t *d_word, uint32_t *d_node,
                                     uint32_t *d_bow_id, double *d_bow_val, int32_t *d_n_bow, uint32_t *d_fv_node_id,
                                     int32_t *d_fv_start, int32_t *d_fv_idx, int32_t *d_n_fv, void *d_scratch, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * KeyFrameDatabase: the inverted file (KeyFrameDatabase.cc:39-98) and its two live queries,
 * DetectRelocalizationCandidates (KeyFrameDatabase.cc:814-926, called at Tracking.cc:3772) and DetectNBestCandidates
 * (KeyFrameDatabase.cc:620-811, called at LoopClosing.cc:519), over mpVoc->score = L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  It consumes the BowVector that orbv_transform leaves and names the
 * candidates that orbm_search_by_bow_candidates / orbm_search_by_bow_keyframes_candidates take.  DetectLoopCandidates,
 * DetectCandidates and DetectBestCandidates have no call site in the reference and are not covered.  The arithmetic is stated
 * once, in csrc/orb_ref_kfdb.h, for the host forms and the kernels (csrc/orb_kfdb_kernels.h); everything is bit-exact against the
 * literal model of tests/kfdb_model.py (reference text unpinned: nothing of KeyFrameDatabase.cc is compiled against it yet).
 *
 * A query has two parts.  The heavy part (orbd_query_*: :816-871, :627-711) counts common words per keyframe, gates at
 * maxCommonWords * 0.8f and scores what passes; it grows with the map and runs on the device.  The small part
 * (orbd_accumulate_*: :873-923, :713-748) accumulates over at most ORBD_COVISIBLES covisibles of each scored keyframe; it reads the
 * caller's live objects (GetBestCovisibilityKeyFrames, and in the take loop isBad / GetMap) and runs on the host.
 *
 * Keyframes are named by `tag`, the caller's opaque 64-bit name (a KeyFrame*, an mnId), unique among live entries; ORBD_NO_TAG is
 * reserved as padding.  Results are always reported as tags, so the handle renumbers its slots when it compacts.
 *
 * The ORDER RULE, next to the MASKING, SEQUENTIAL, INDEPENDENCE, FUSE and SEARCH-AND-FUSE RULES above.  The reference's result
 * order is the order of lKFsSharingWords: the order of first encounter in a walk over the query's words in ascending id and over
 * each word's list in insertion order (:822-837, :639-671).  add (:39-45) appends the keyframe to the list of every one of its
 * words in one call, and erase (:47-66) and clearMap (:74-98) remove without reordering, so EVERY list is a subsequence of the
 * global add order.  A keyframe is first met under the smallest word id it shares with the query, and among the keyframes first
 * met under the same word the list's order - the add order - decides.  Hence the first-encounter key of keyframe i is
 *     (smallest word id it shares with the query, add sequence number of i),
 * and sorting those unique keys gives the list.  Two consequences: a keyframe that is erased and added again moves to the END of
 * its lists (as in the reference: push_back); and the reference's add would list a keyframe twice if it were called twice for it -
 * every path of LoopClosing.cc:314-547 adds once and returns - so a second orbd_add of a live tag is refused.
 *
 * Query state.  The four KeyFrame members that only KeyFrameDatabase.cc reads or writes (serialisation apart) - mnRelocQuery,
 * mRelocScore, mnPlaceRecognitionQuery, mPlaceRecognitionScore - live in host arrays of the handle, 0 for a new entry unless
 * orbd_add is given values (PostLoad); orbd_get_members reads them back for a saved map.  The accumulation adds scores left by
 * EARLIER queries for a neighbour that was listed but did not pass the gate this time (:888-891, :730-733); holding the members
 * here keeps that exact.  DEVIATION: the reference leaves mRelocScore uninitialised (KeyFrame.cc:34, :52), so reading it before
 * the first write is an uninitialised read there; here it is 0.  mnRelocWords / mnPlaceRecognitionWords are not kept: a count
 * is only ever read of a keyframe the same query listed, and listing resets it (:831, :655).
 * A keyframe whose stored query id already EQUALS query_id is not listed again (:829, :653) - which is why query id 0 finds
 * nothing in fresh entries until another query has run.  In the place form a connected keyframe is counted but never listed and
 * never marked (:653-663): it is absent from maxCommonWords, from the list and from the later neighbour test.
 *
 * Every entry validates everything before anything is written or launched, takes the handle's mutex where the reference holds
 * mMutex (so Tracking, LocalMapping and LoopClosing threads may share a handle), and returns 0, ORBX_E_ARG or ORBX_E_HIP with the
 * reason in orbd_last_error (per calling thread).
 * ------------------------------------------------------------------------------------------------------------------ */
#define ORBD_MAX_KEYFRAMES 16384            /* live keyframes: what one workgroup sorts in LDS (csrc/orb_sort.h) */
#define ORBD_COVISIBLES 10                  /* GetBestCovisibilityKeyFrames(10), :880, :722 */
#define ORBD_NO_TAG 0xffffffffffffffffull   /* pads a covisibles row */

typedef struct orbd_handle orbd_t;

typedef struct {
  uint64_t reloc_query;   /* mnRelocQuery */
  uint64_t place_query;   /* mnPlaceRecognitionQuery */
  float reloc_score;      /* mRelocScore */
  float place_score;      /* mPlaceRecognitionScore */
} orbd_members_t;

/* KeyFrameDatabase::KeyFrameDatabase (KeyFrameDatabase.cc:32-36) for a vocabulary of n_words words.  scoring: only 0 (L1_NORM, what
 * ORBvoc uses; BowVector.h:48-56) is accepted.  capacity: live keyframes, in [1, ORBD_MAX_KEYFRAMES].  device >= 0 allocates the
 * device tables; device = -1 gives a handle on which only the host forms work (for tests without a GPU; it is no fallback:
 * the device entries return ORBX_E_ARG on it).  NULL on failure, the reason in orbd_last_error(NULL).
 * orbd_create_for_vocabulary takes n_words and the scoring from a vocabulary. */
orbd_t *orbd_create(int n_words, int scoring, int capacity, int device);
orbd_t *orbd_create_for_vocabulary(const orbv_t *v, int capacity, int device);
void orbd_destroy(orbd_t *d);
const char *orbd_last_error(const orbd_t *d);
int orbd_n_words(const orbd_t *d);
int orbd_capacity(const orbd_t *d);
int orbd_size(orbd_t *d);   /* live keyframes */

/* KeyFrameDatabase::add (KeyFrameDatabase.cc:39-45): appends the keyframe's BowVector bow_id[n] (strictly ascending, below n_words),
 * bow_val[n] (finite).  init: the four members (PostLoad) or NULL for zeros.  ORBX_E_ARG: an invalid vector, a duplicate tag,
 * ORBD_NO_TAG, `capacity` live keyframes.  On the device the vectors are a CSR in add order (word ids, double values); erased
 * entries are tombstones until a compaction, which keeps the relative order of the live entries and is invisible to the caller.
 * orbd_add_device takes the vector of frame p of an orbv_transform_batch_device output (d_bow_id / d_bow_val [..][cap], d_n_bow[..])
 * by device-to-device copies on `stream` and reads back only the 4-byte count; it returns after the copies.  Such an entry has no
 * host copy, so the host forms refuse a handle that holds one. */
int orbd_add(orbd_t *d, uint64_t tag, uint64_t map_id, const uint32_t *bow_id, const double *bow_val, int n, const orbd_members_t *init);
int orbd_add_device(orbd_t *d, uint64_t tag, uint64_t map_id, const uint32_t *d_bow_id, const double *d_bow_val, const int32_t *d_n_bow,
                    int cap, int p, const orbd_members_t *init, void *stream);
/* KeyFrameDatabase::erase (:47-66), clear (:68-72), clearMap (:74-98).  orbd_set_map: a merge moves keyframes between maps
 * (the reference reads pKF->GetMap() when it needs it, :87, :915). */
int orbd_erase(orbd_t *d, uint64_t tag);
int orbd_clear(orbd_t *d);
int orbd_clear_map(orbd_t *d, uint64_t map_id);
int orbd_set_map(orbd_t *d, uint64_t tag, uint64_t map_id);
int orbd_get_members(orbd_t *d, uint64_t tag, orbd_members_t *out);

/* The heavy part of DetectRelocalizationCandidates (KeyFrameDatabase.cc:816-871) and of DetectNBestCandidates
 * (KeyFrameDatabase.cc:627-711) for the query BowVector bow_id[n], bow_val[n] (as orbd_add; n in [0, ORBM_MAX_KEYPOINTS]).
 *   query_id                     F->mnId / pKF->mnId
 *   connected_tags[n_connected]  pKF->GetConnectedKeyFrames() (:637), place form; every tag must be in the database
 *   out_tag, out_score [out_cap] lScoreAndMatch in the reference's order (ORDER RULE): the first *n_scored entries;
 *                                out_cap >= orbd_size(d)
 *   *max_common, *min_common     maxCommonWords, minCommonWords = (int)(maxCommonWords * 0.8f); a keyframe is scored when its count
 *                                is strictly greater
 *   *n_listed                    lKFsSharingWords.size()
 * score: over the word ids in both vectors, ascending, `score += fabs(vi - wi) - fabs(vi) - fabs(wi)` in double with vi the
 * query's value and wi the keyframe's, then -score / 2.0 rounded to float (ScoringObject.cpp:32-65).  The stored query ids and
 * scores are updated as the reference updates the members (:832, :865, :659, :705).
 * The device forms cost one upload of the query, one download of the compact result and one synchronisation.  The _host forms
 * run csrc/orb_ref_kfdb.h in plain C++ over the handle's host copy; they exist for tests, like orbv_transform_host. */
int orbd_query_reloc(orbd_t *d, uint64_t query_id, const uint32_t *bow_id, const double *bow_val, int n, uint64_t *out_tag, float *out_score,
                     int out_cap, int32_t *n_scored, int32_t *max_common, int32_t *min_common, int32_t *n_listed);
int orbd_query_reloc_host(orbd_t *d, uint64_t query_id, const uint32_t *bow_id, const double *bow_val, int n, uint64_t *out_tag,
                          float *out_score, int out_cap, int32_t *n_scored, int32_t *max_common, int32_t *min_common, int32_t *n_listed);
int orbd_query_place(orbd_t *d, uint64_t query_id, const uint64_t *connected_tags, int n_connected, const uint32_t *bow_id,
                     const double *bow_val, int n, uint64_t *out_tag, float *out_score, int out_cap, int32_t *n_scored, int32_t *max_common,
                     int32_t *min_common, int32_t *n_listed);
int orbd_query_place_host(orbd_t *d, uint64_t query_id, const uint64_t *connected_tags, int n_connected, const uint32_t *bow_id,
                          const double *bow_val, int n, uint64_t *out_tag, float *out_score, int out_cap, int32_t *n_scored,
                          int32_t *max_common, int32_t *min_common, int32_t *n_listed);

/* The relocalisation query (KeyFrameDatabase.cc:816-871) for `nq` resident BowVectors in the layout orbv_transform_batch_device writes
 * (d_bow_id / d_bow_val [nq][cap], d_n_bow[nq]; query q has min(max(d_n_bow[q], 0), cap) words), asynchronous on `stream`: the same
 * kernels with a grid over all queries.  query_id[nq] is a HOST array, one id per query: a keyframe whose stored mnRelocQuery
 * equals it is not listed.  It READS the handle's arrays and does NOT update them: no keyframe is marked and no score is stored.
 * Per query it writes d_out_tag / d_out_score [nq][out_cap] (the scored list in list order; out_cap in [max(orbd_size, 1), capacity])
 * and d_counts[nq][4] = maxCommonWords, minCommonWords, keyframes scored, keyframes listed.  d_scratch:
 * orbd_batch_scratch_bytes(d, nq) bytes, 8-byte aligned, that belong to the call until the stream has passed it; the handle must not
 * be changed (add, erase, clear, queries) until then. */
size_t orbd_batch_scratch_bytes(const orbd_t *d, int nq);
int orbd_score_batch_device(orbd_t *d, int nq, const uint64_t *query_id, const uint32_t *d_bow_id, const double *d_bow_val,
                            const int32_t *d_n_bow, int cap, uint64_t *d_out_tag, float *d_out_score, int out_cap, int32_t *d_counts,
                            void *d_scratch, void *stream);

/* The small part.  tags / scores [n]: a query's scored list; covisibles[n][ORBD_COVISIBLES]: GetBestCovisibilityKeyFrames(10) of
 * each, as tags, padded with ORBD_NO_TAG.  A neighbour that is unknown to the handle or erased counts as "query id differs" and is
 * skipped; a scored tag must be in the database.
 * orbd_accumulate_reloc (KeyFrameDatabase.cc:873-923): the float accumulation in the reference's order, pBestKF, bestAccScore,
 * 0.75f * bestAccScore and the strict `>`; the map filter (:915) is applied AFTER the threshold was computed over all maps; no
 * duplicates, list order.  out_tags[n], *n_out.
 * orbd_accumulate_place (KeyFrameDatabase.cc:713-748): the same accumulation, then list::sort(compFirst): stable, descending by
 * accumulated score.  out_acc[n], out_best[n]: the whole sorted list; the take loop of :760-783 stays with the caller. */
int orbd_accumulate_reloc(orbd_t *d, uint64_t query_id, uint64_t map_id, const uint64_t *tags, const float *scores, int n,
                          const uint64_t *covisibles, uint64_t *out_tags, int32_t *n_out);
int orbd_accumulate_place(orbd_t *d, uint64_t query_id, const uint64_t *tags, const float *scores, int n, const uint64_t *covisibles,
                          float *out_acc, uint64_t *out_best);

#ifdef __cplusplus
}
#endif
#endif /* ORBHIP_H */
