/*
 * find_motion_amd.h — C ABI of the MI355X motion-detection hot path.
 *
 * The reference (dmiruke/find_motion, find_motion/find_motion.py = "fm.py")
 * has no FFI: its hot path is a chain of cv2 calls made from three
 * VideoMotion methods in the frame loop (fm.py:866-868):
 *
 *   blur_frame()      fm.py:487-494  imutils.resize -> cvtColor -> GaussianBlur
 *   mask_off_areas()  fm.py:619-636  rectangle / fillConvexPoly onto frame.blur
 *   find_diff()       fm.py:638-662  convertScaleAbs+absdiff, threshold,
 *                                    accumulateWeighted, dilate, findContours
 *
 * This header is the boundary a binding (ctypes / cffi / pybind11) would bind
 * to replace those three methods; find_motion_amd/motion.py is that binding.
 * Every entry point is a plain C function over plain pointers and sizes.
 * Status codes: 0 = OK, negative = error (see FM_E*); fm_last_error() gives
 * the message.  No C++ exception crosses this boundary.
 *
 * Threading: one fm_ctx per host thread; contexts are independent and bound
 * to one HIP device (one process per GPU in the multi-GPU runner).
 */
#ifndef FIND_MOTION_AMD_H
#define FIND_MOTION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_ABI_VERSION 1

/* status codes */
#define FM_OK 0
#define FM_EINVAL -1   /* bad argument */
#define FM_EHIP -2     /* HIP runtime error */
#define FM_ENOMEM -3   /* allocation failed */
#define FM_ESTATE -4   /* call out of order (e.g. results before fm_wait) */
#define FM_ENOTSUP -5  /* configuration outside the restated OpenCV path */

/* fm_params.flags */
#define FM_FLAG_KEEP_PLANES 0x1u /* keep gray/blur/frame_delta per frame (show/debug, fm.py:907-926) */
#define FM_FLAG_PROFILE 0x2u     /* time every kernel launch with HIP events */
#define FM_FLAG_PROFILE_PIX 0x4u /* time only the pixel-stream kernels (cheap enough for the bench's timed loop) */
#define FM_FLAG_CONTOUR_AREA 0x8u /* trace every external contour's border on the GPU at fm_wait and return
                                     2 x cv2.contourArea (fm.py:679) in fm_contour.area2: needed only where
                                     the area filter of fm.py:684 is live (max_area < min_area) */
#define FM_FLAG_CONTOUR_POINTS 0x10u /* trace every external contour's border on the GPU at fm_wait and keep its
                                        CHAIN_APPROX_SIMPLE points, the arrays cv2.findContours returns
                                        (fm.py:269-272): fm_contour.npts, fm_get_contour_points.  area2 is filled
                                        too (the count pass has it; FM_FLAG_CONTOUR_AREA need not be set and
                                        starts no second trace).  Off: no kernel, buffer or result differs */
#define FM_FLAG_AREA_UPSCALE 0x20u /* accept box_size > src_w: imutils.resize(raw, width=box) enlarges the frame
                                      (fm.py:490), and cv2.resize(INTER_AREA) then runs its 8-bit bilinear resizer
                                      with area-mode taps (the kernel `resize_area_up`).  Off: FM_ENOTSUP for such
                                      a box, as before; no kernel, buffer, result or status differs */
#define FM_FLAG_COLOUR_MOTION 0x40u /* detect motion per colour channel: the chain the reference would run without
                                       its cvtColor line (fm.py:493; the TODO at the top of find_motion.py).
                                       GaussianBlur per channel, the keep-mask zeroes all three, absdiff /
                                       convertScaleAbs / accumulateWeighted run element-wise over [h][w][3] (their
                                       SIMD rules count 3hw elements), and a pixel is set where any channel's
                                       delta exceeds the threshold; dilation, contours, boxes and points as
                                       always.  A mover whose gray level equals the background's is seen.  The
                                       kernels `rgb_blur` + `rgb_scan`; the background has 3 doubles per pixel
                                       (fm_background_channels).  FM_ENOTSUP with ksize above 49, more than 8,192
                                       tiles, or FM_FLAG_KEEP_PLANES (FM_PLANE_SMALL still works).  Off: no
                                       kernel, buffer, result or status differs */
#define FM_FLAG_MOG2 0x80u /* a Gaussian-mixture background model in place of the running average: what
                              `fgmask = cv2.createBackgroundSubtractorMOG2(...).apply(frame.blur)` gives in
                              find_diff (fm.py:638-662), one channel, five mixtures.  Resize, gray, GaussianBlur and
                              the keep-mask as always; then a pixel is set where the mask value is 255 (a shadow, 127,
                              is not foreground); dilation, contours, boxes and points as always.  threshold and avg
                              are not used.  A pixel that alternates between two values is learnt and stays silent.
                              The kernels `small_blur` or `wide_blur` + `mog2_scan`; fm_plan says "mog2".
                              Parameters: fm_create_mog2 (fm_create takes the defaults).  FM_ENOTSUP with
                              FM_FLAG_COLOUR_MOTION, FM_FLAG_KEEP_PLANES, more than 8,192 tiles, or a ksize neither
                              blur takes (ksize 1 on more than 16,384 work pixels).  Off: no kernel, buffer, result
                              or status differs */

/* planes for fm_read_plane */
#define FM_PLANE_GRAY 0  /* VideoFrame.gray        (fm.py:493) */
#define FM_PLANE_BLUR 1  /* VideoFrame.blur, masked (fm.py:494, 619-636) */
#define FM_PLANE_DELTA 2 /* VideoFrame.frame_delta (fm.py:250) */
#define FM_PLANE_SMALL 3 /* the INTER_AREA-resized BGR frame `small` (fm.py:490), h*w*3 bytes; resize modes only
                            (the enlarged frame under FM_FLAG_AREA_UPSCALE), no FM_FLAG_KEEP_PLANES needed */

typedef struct fm_ctx fm_ctx;

/* Construction parameters: the VideoMotion constructor arguments that reach
 * the hot path (fm.py:299-307) plus the batch geometry. */
typedef struct fm_params {
    int device;       /* HIP device ordinal */
    int n_streams;    /* independent videos/cameras, one background model each */
    int src_w, src_h; /* decoded frame size (fm.py:433-435) */
    int box_size;     /* -B / box_size: processing width (fm.py:492, 1474) */
    int ksize;        /* odd Gaussian size from _make_gaussian (fm.py:478-484) */
    int threshold;    /* -t / threshold (fm.py:256, 1476) */
    double avg;       /* -a / avg, accumulateWeighted alpha (fm.py:659, 1479) */
    int max_batch;    /* max frames per stream per fm_submit */
    int max_contours; /* per-frame contour records kept in mapped host memory (a frame
                         with more is fetched whole at fm_wait: no contour is lost) */
    unsigned flags;   /* FM_FLAG_* */
} fm_params;

/* One external contour (an element of VideoFrame.contours, fm.py:269-276). */
typedef struct fm_contour {
    int32_t x, y, w, h;          /* cv2.boundingRect (fm.py:792) */
    int32_t origin_x, origin_y;  /* border start = raster-first pixel of the component */
    int32_t area2;               /* 2 x cv2.contourArea of the CHAIN_APPROX_SIMPLE contour (an integer: the
                                    shoelace sum); -1 unless the context has FM_FLAG_CONTOUR_AREA or
                                    FM_FLAG_CONTOUR_POINTS */
    int32_t npts;                /* its number of CHAIN_APPROX_SIMPLE points (>= 1); 0 unless the context has
                                    FM_FLAG_CONTOUR_POINTS */
} fm_contour;

/* Library version (FM_ABI_VERSION) */
int fm_abi_version(void);

/* Create / destroy a context.  Allocates all device state. */
int fm_create(fm_ctx** out, const fm_params* params);
void fm_destroy(fm_ctx* ctx);

/* Parameters of the Gaussian-mixture background model (FM_FLAG_MOG2): BackgroundSubtractorMOG2's, with OpenCV's
 * defaults from fm_mog2_defaults.  nmixtures is fixed at 5. */
typedef struct fm_mog2_params {
    int history;                /* 500: frames until the learning rate settles at 1 / history */
    float var_threshold;        /* 16 (Tb): squared distance in variances below which a mode explains the pixel */
    float var_threshold_gen;    /* 9 (Tg): ... below which the pixel updates the mode */
    float background_ratio;     /* 0.9 (TB): summed weight of the modes that count as background */
    float var_init;             /* 15 */
    float var_min;              /* 4 */
    float var_max;              /* 75 */
    float complexity_reduction; /* 0.05 (CT): prior that prunes weak modes */
    float shadow_tau;           /* 0.5: darkest shadow as a fraction of the background */
    int detect_shadows;         /* 1: mark shadows 127 (not foreground) */
    double learning_rate;       /* -1: automatic, 1 / min(2 nframes, history); else the rate from the 2nd frame on */
} fm_mog2_params;
int fm_mog2_defaults(fm_mog2_params* out);
/* fm_create with FM_FLAG_MOG2 set and these parameters (NULL: the defaults, which is what fm_create gives when the
 * flag is set).  FM_EINVAL, before any device call, for history < 1, a non-finite or negative float, var_min >
 * var_max, background_ratio outside (0, 1] or learning_rate > 1; FM_ENOTSUP as the flag describes. */
int fm_create_mog2(fm_ctx** out, const fm_params* params, const fm_mog2_params* mog2);

/* What fm_create would set up for params, without touching a device: the same validation (and error codes)
 * and the same selection, by the same code.  pixel_path names the kernels of the per-pixel chain:
 *   "small"  k_small_blur + k_small_scan (work images of at most 16,384 pixels, ksize up to 49)
 *   "pix"    k_pix (ksize 3, 5, 7, 21)
 *   "fused"  k_fused (other ksize up to 49)
 *   "wide"   k_wide_blur + k_small_scan (ksize above 49, more than 16 and at most 8,192 tiles of 64 x 64,
 *            no FM_FLAG_KEEP_PLANES)
 *   "rgb"    k_rgb_blur + k_rgb_scan (FM_FLAG_COLOUR_MOTION: ksize up to 49, at most 8,192 tiles)
 *   "mog2"   k_small_blur or k_wide_blur + k_mog2_scan (FM_FLAG_MOG2: at most 8,192 tiles)
 *   "pixel"  one k_pixel launch per frame and the pixel-level CCL: one batch in flight
 * (The struct has no typedef: C keeps struct tags apart from function names, not typedef names.) */
struct fm_plan {
    int32_t work_h, work_w; /* fm_work_size */
    int32_t tiles;          /* 64 x 64 tiles of the work image */
    int32_t max_inflight;   /* fm_max_inflight */
    char pixel_path[16];
};
int fm_plan(const fm_params* params, struct fm_plan* out);

/* Which resize fm_create would set up in front of the pixel chain, without touching a device; fm_plan's
 * validation and status codes (FM_RESIZE_UP only with FM_FLAG_AREA_UPSCALE, FM_ENOTSUP for such a box without). */
#define FM_RESIZE_IDENTITY 0 /* box_size = src_w: the frame is the work image */
#define FM_RESIZE_FAST 1     /* INTER_AREA by whole factors */
#define FM_RESIZE_GENERAL 2  /* INTER_AREA, any shrinking factors */
#define FM_RESIZE_UP 3       /* box_size > src_w: the enlarging resize */
int fm_resize_kind(const fm_params* params, int* kind);
/* The enlarging resize's taps for one axis of ssize source and dsize >= ssize destination elements, as the engine
 * and the detectors build them (host only): per destination index the two source indices and their 11-bit
 * coefficients (a0 + a1 = 2048), dsize values each. */
int fm_area_up_taps(int ssize, int dsize, int32_t* s0, int32_t* s1, int32_t* a0, int32_t* a1);
/* The 8-bit fixed-point Gaussian taps every pixel path blurs with at this ksize (host only): ksize values that
 * sum to 256.  FM_EINVAL for an even ksize, one below 1 or above 255, or a null pointer; out is then untouched. */
int fm_gaussian_taps(int ksize, int32_t* out);

/* Last error message for ctx (or the calling thread's last error if ctx is NULL). */
const char* fm_last_error(const fm_ctx* ctx);

/* Working image size (h = int(src_h * box/src_w), w = box; imutils rule, fm.py:492). */
int fm_work_size(const fm_ctx* ctx, int* h, int* w);

/* Static keep-mask for one stream: h*w bytes, 0 = masked off (mask_off_areas,
 * fm.py:619-636, rasterised once per video).  NULL clears the mask. */
int fm_set_mask(fm_ctx* ctx, int stream, const uint8_t* keep_hw);

/* Forget the background model: the next frame re-initialises it
 * (VideoMotion.ref_frame = None, fm.py:414, 651-652).  With FM_FLAG_MOG2: nmodes = 0 everywhere and nframes = 0. */
int fm_reset_stream(fm_ctx* ctx, int stream);

/* Batches that may be in flight at once (fm_submit before fm_wait): the contour
 * pass of one batch overlaps the pixel kernel of the next ones. */
int fm_max_inflight(const fm_ctx* ctx);

/* Run the hot path on n_frames consecutive frames of every stream.
 * frames: BGR u8, layout [n_frames][n_streams][src_h][src_w][3], C-contiguous;
 * host memory (on_device = 0, copied with hipMemcpyAsync) or device memory
 * (on_device = 1, read in place).  Asynchronous: host buffers must stay valid
 * until fm_wait returns for this batch.  Up to fm_max_inflight() batches may be
 * submitted before waiting; fm_wait completes them in submission order. */
int fm_submit(fm_ctx* ctx, const uint8_t* frames, int n_frames, int on_device);

/* fm_submit with one frame pointer per stream, SURVEY.md §8(b)'s
 * fm_submit(ctx, const uint8_t* const* bgr, n_frames): bgr[s] holds stream s's
 * n_frames consecutive frames [n_frames][src_h][src_w][3] (e.g. what a
 * per-stream decoder wrote).  Host memory: one strided DMA per stream puts them
 * into the batch's [t][s] layout on the input stream (no gather copy on the
 * host; page-locked buffers make it asynchronous).  Device memory: read in
 * place for one stream, one strided device copy per stream otherwise.
 * Results are identical to fm_submit of the same frames gathered into
 * [n_frames][n_streams] order; the same lifetime rules apply. */
int fm_submit_streams(fm_ctx* ctx, const uint8_t* const* bgr, int n_frames, int on_device);

/* Page-locked host memory for frame batches (a decoder writes frames here): fm_submit
 * of such a buffer is a true asynchronous DMA (hipMemcpyAsync) on the context's input
 * stream, overlapped with the previous batch's kernels (north_star: "frame batches
 * pinned and hipMemcpyAsync-overlapped with compute").  Replaces nothing in the
 * reference (cap.read() returns pageable numpy frames, fm.py:501); optional. */
int fm_host_alloc(fm_ctx* ctx, size_t bytes, void** out);
int fm_host_free(fm_ctx* ctx, void* ptr);

/* Wait for the oldest batch in flight; makes its results readable (device-side
 * results -- masks, planes -- until that batch's slot is reused by a later submit). */
int fm_wait(fm_ctx* ctx);

/* External-contour counts of the last batch, layout [n_frames][n_streams]
 * (len(VideoFrame.contours), the quantity find_movement counts, fm.py:674-695). */
int fm_get_counts(fm_ctx* ctx, int32_t* counts);

/* Contours of one (frame, stream) of the last batch, in raster order of their
 * start pixels.  Returns the count (records written: min(count, cap)).  Every
 * contour is kept whatever fm_params.max_contours is (a frame with more is
 * fetched whole by fm_wait), so a second call with cap = count gets them all. */
int fm_get_contours(fm_ctx* ctx, int frame, int stream, fm_contour* out, int cap);

/* FM_FLAG_CONTOUR_POINTS: the CHAIN_APPROX_SIMPLE points of every contour of one (frame, stream) of the last
 * batch, xy = [*total][2] as (x, y).  Contours in the order of fm_get_contours: contour i's npts_i points
 * follow those of contours 0 .. i-1; within a contour in trace order, the order cv2.findContours returns,
 * first point the start pixel (origin_x, origin_y).  *total is always set; the points are copied when
 * cap >= *total (cap counts points), FM_EINVAL otherwise: call again with *total, as fm_mjpeg_enc_get.
 * FM_ESTATE without the flag or before the first fm_wait.  A host copy: fm_wait fetched the whole batch's
 * points in one transfer.  Valid until the next fm_wait, like the records.
 * Limits: fewer than 2^31 points and about 1.7e8 contours per batch (FM_ENOMEM from fm_wait beyond); a
 * start pixel whose border does not close within 4 (w + 2)(h + 2) + 16 steps makes fm_wait return FM_EHIP. */
int fm_get_contour_points(fm_ctx* ctx, int frame, int stream, int32_t* xy, size_t cap, size_t* total);
/* Diagnostics of the last waited batch's contour trace: contours traced from a staged window (registers or
 * LDS: padded box up to 63.5 KiB of bit rows, about 700 x 700), contours traced unstaged (larger
 * boxes: global memory behind a sliding window), and the border steps walked by the count pass. */
int fm_last_trace_stats(const fm_ctx* ctx, int32_t* staged, int32_t* unstaged, int64_t* steps);

/* Diagnostics: frames of the last waited batch whose contours came from the
 * pixel-level fallback (the batch exhausted its contour-pass node pool). */
int fm_last_fallbacks(const fm_ctx* ctx);
/* Diagnostics of the last waited batch's contour pass: union-find nodes its frames
 * took from the shared pool (past their own quotas) and tiles labelled by the heavy
 * pass (more than 256 runs: dense speckle). */
int fm_last_ccl_stats(const fm_ctx* ctx, int32_t* shared_nodes, int32_t* heavy_tiles);

/* Dilated threshold mask (VideoFrame.thresh after find_contours, fm.py:266), h*w bytes. */
int fm_read_mask(fm_ctx* ctx, int frame, int stream, uint8_t* out);

/* Diagnostics: the undilated threshold bits (frame_delta > threshold, fm.py:257) as the tile pixel paths
 * store them: for each 64 x 64 tile of the work image in raster order, 64 column words (word c, bit r =
 * pixel (row r, column c) of the tile), ntiles * 64 words in all; bits past the image are zero.
 * FM_ESTATE on the paths that keep no threshold bits (Gaussian sizes the tile kernels do not take). */
int fm_read_threshold_bits(fm_ctx* ctx, int frame, int stream, uint64_t* out);

/* gray / blur / frame_delta planes (needs FM_FLAG_KEEP_PLANES), h*w bytes; FM_PLANE_SMALL: the
 * resized BGR frame, h*w*3 bytes (FM_ESTATE when box_size = frame width). */
int fm_read_plane(fm_ctx* ctx, int plane, int frame, int stream, uint8_t* out);

/* Background model (VideoMotion.ref_frame, float64, fm.py:652, 659), h*w doubles; on a context with
 * FM_FLAG_COLOUR_MOTION 3*h*w doubles in [h][w][3] order (B, G, R), the numpy array it would be. */
int fm_read_background(fm_ctx* ctx, int stream, double* out);
int fm_write_background(fm_ctx* ctx, int stream, const double* in);
/* Doubles per work pixel of the background: 1, or 3 with FM_FLAG_COLOUR_MOTION. */
int fm_background_channels(const fm_ctx* ctx, int* channels);
/* On a context with FM_FLAG_MOG2 the three calls above give FM_ESTATE (there is no average); the calls below give
 * FM_ESTATE on any other context, and while a batch is in flight.
 * The model of one stream: weight, mean, var [5][h][w] floats row-major, nmodes [h][w] (0..5), nframes the frames
 * the stream has seen.  Entries at mode >= nmodes read as 0 and are ignored when written; a written nmodes above 5
 * is FM_EINVAL.  For tests, and for carrying a model from one file of a camera to the next. */
int fm_mog2_read_model(fm_ctx* ctx, int stream, float* weight, float* mean, float* var, uint8_t* nmodes, int64_t* nframes);
int fm_mog2_write_model(fm_ctx* ctx, int stream, const float* weight, const float* mean, const float* var,
                        const uint8_t* nmodes, const int64_t* nframes);
/* getBackgroundImage of one stream, h*w bytes: the weighted mean of the strongest modes up to background_ratio,
 * 0 where a pixel has no mode yet. */
int fm_mog2_background(fm_ctx* ctx, int stream, uint8_t* out_hw);

/* Launch on the caller's HIP stream (hipStream_t) instead of the context's own
 * stream; NULL restores the context stream.  FM_ESTATE while a batch is in flight.
 *
 * Ordering.  On a caller's stream every fm_submit* call is ordered after the work
 * the caller queued on that stream before the call: device input (fm_submit /
 * fm_submit_streams / fm_submit_yuv with on_device = 1, fm_submit_yuv_list) may
 * still be being written by a decode or copy queued there, with no host
 * synchronisation.  The context keeps its private input stream for the copies,
 * the YUV conversion and the INTER_AREA resize; that stream first waits for an
 * event recorded on the caller's stream.  Work the caller queues on its stream
 * after the call runs after the batch's pixel kernels, which have read the input
 * by then (the contour pass runs on the context's other streams: results are
 * read after fm_wait, as always).  On the context's own stream nothing orders a
 * batch against the caller's streams: device input must be complete before the
 * call.  The caller keeps ownership of its stream; fm_destroy synchronises it
 * and leaves it usable. */
int fm_set_hip_stream(fm_ctx* ctx, void* hip_stream);

/* Memory the context holds: device bytes (fm_create's buffers, plus input staging allocated on the
 * first host submit) and page-locked host bytes (the mapped contour records and counters).  No
 * reference counterpart (sizing for many streams per GPU). */
int fm_footprint(const fm_ctx* ctx, size_t* device_bytes, size_t* pinned_bytes);

/* FM_FLAG_PROFILE: per-kernel accumulated device time since the last reset.
 * names[i] (static strings), ms[i], launches[i] for i < returned count. */
int fm_kernel_times(fm_ctx* ctx, const char** names, double* ms, int64_t* launches, int cap);
/* The same kernels in the same order, with ms_sq[i] = the sum of the squared launch times (ms^2) of the
 * launches timed by in-kernel stamps (the pixel kernel and the INTER_AREA resize under FM_FLAG_PROFILE_PIX;
 * 0 for event-timed kernels), for the spread of the launch time across a run. */
int fm_kernel_time_spread(fm_ctx* ctx, double* ms_sq, int cap);
/* The same kernels in the same order, with busy_ms[i] = the time during which at least one of the kernel's
 * stamped launches was running (the union of their windows; less than the summed launch times when launches
 * of one kernel overlap, e.g. the resizes of consecutive batches on the two input streams). */
int fm_kernel_time_busy(fm_ctx* ctx, double* busy_ms, int cap);
/* Everything above from ONE fold of the launch stamps (so the sums, the squares and the counts cover the same
 * launches): per kernel ms and launches (stamped + event-timed), stamped_ms / stamped / ms_sq (the stamped
 * launches alone: their sum, count and sum of squares, for the spread), busy_ms; *unstamped = launches that
 * found the stamp ring full between two folds (event-timed on one launch in four, or untimed).  Any array may
 * be NULL. */
int fm_kernel_time_stats(fm_ctx* ctx, const char** names, double* ms, int64_t* launches, double* stamped_ms,
                         int64_t* stamped, double* ms_sq, double* busy_ms, int64_t* unstamped, int cap);
int fm_reset_kernel_times(fm_ctx* ctx);

/* Rasterise mask polygons to a keep-mask (mask_off_areas, fm.py:611-636):
 * each polygon's points are scaled by int(v * scale) (scale_area, fm.py:616);
 * 2 points -> filled rectangle (cv2.rectangle FILLED), >= 3 points ->
 * cv2.fillConvexPoly.  xy: all points (x0,y0,x1,y1,...), npts: points per
 * polygon.  keep (h*w) is set to 1 everywhere, then 0 inside the polygons. */
int fm_rasterize_masks(int h, int w, double scale, const int32_t* xy, const int32_t* npts,
                       int n_polys, uint8_t* keep);

/* ---- Object-ROI stage ----------------------------------
 * Replaces cv2.CascadeClassifier(path) + detectMultiScale(frame.resized,
 * scaleFactor=1.1, minNeighbors=5) at find_motion.py:396 and :722-731 for HAAR
 * cascades (find_motion_amd/cascade.py reads the XML into this description).
 * Independent of fm_ctx: one detector per cascade and device. */
typedef struct fm_haar fm_haar;
typedef struct fm_haar_desc {
    int win_w, win_h;                /* <width>, <height> */
    int n_stages, n_trees, n_nodes, n_leaves, n_features;
    const int32_t* stage_ntrees;     /* [n_stages] weak classifiers per stage */
    const float* stage_threshold;    /* [n_stages] (float)value - 1e-5f, as Data::read */
    const int32_t* tree_nodes;       /* [n_trees] internal nodes per tree */
    const int32_t* node_left;        /* [n_nodes] > 0: node of the same tree, <= 0: leaf -v */
    const int32_t* node_right;       /* [n_nodes] */
    const int32_t* node_feature;     /* [n_nodes] feature index */
    const float* node_threshold;     /* [n_nodes] */
    const float* leaves;             /* [n_leaves] = tree nodes + 1 per tree */
    const int32_t* feat_rects;       /* [n_features][3][4] x y w h */
    const float* feat_weights;       /* [n_features][3], 0 = unused third rect */
    const uint8_t* feat_tilted;      /* [n_features] or NULL */
} fm_haar_desc;

/* Validate and upload a cascade (FM_EINVAL before any HIP call when the
 * description is inconsistent).  *out is set even on failure so that
 * fm_haar_last_error can say why; release it with fm_haar_destroy. */
int fm_haar_create(int device, const fm_haar_desc* desc, fm_haar** out);
void fm_haar_destroy(fm_haar* det);
const char* fm_haar_last_error(const fm_haar* det);
int fm_haar_window(const fm_haar* det, int* w, int* h);

/* detectMultiScale over n images of one size ([n][H][W][channels] u8, BGR or
 * gray; host memory, or device memory when on_device).  max_w/max_h 0 = the
 * image size.  rects: [n][cap][4] (x, y, w, h), counts[n] = detections per
 * image (may exceed cap; only cap are written).  Synchronous. */
int fm_haar_detect(fm_haar* det, const uint8_t* images, int n, int H, int W, int channels, int on_device,
                   double scale_factor, int min_neighbors, int min_w, int min_h, int max_w, int max_h,
                   int32_t* rects, int cap, int32_t* counts);
/* find_objects (find_motion.py:703-731) on raw frames: each [H][W][3] BGR
 * frame is resized to width roi_w with INTER_AREA on the device
 * (imutils.resize: height int(H * roi_w / W), *roi_h_out), then detected as
 * fm_haar_detect with default min/max sizes.  FM_ENOTSUP when W < roi_w, unless
 * fm_haar_set_roi_upscale allowed it. */
int fm_haar_set_roi_upscale(fm_haar* det, int on); /* on: frames narrower than roi_w are enlarged as
                                                      FM_FLAG_AREA_UPSCALE enlarges them; off (default): refused */
int fm_haar_detect_frames(fm_haar* det, const uint8_t* frames, int n, int H, int W, int on_device, int roi_w,
                          double scale_factor, int min_neighbors, int32_t* rects, int cap, int32_t* counts,
                          int* roi_h_out);
/* fm_haar_detect_frames over n frames already in device memory at n separate
 * addresses (frames[i]: [H][W][3] BGR; the frame list find_objects collects
 * over many streams and batches, fm.py:703-731): the INTER_AREA resize reads
 * each frame where it lies (no gather copy) whenever the tap table has at most
 * 32 taps, and gathers the frames on the detector's stream otherwise. */
int fm_haar_detect_frame_list(fm_haar* det, const uint8_t* const* frames, int n, int H, int W, int roi_w,
                              double scale_factor, int min_neighbors, int32_t* rects, int cap, int32_t* counts,
                              int* roi_h_out);
/* fm_haar_detect_frame_list without waiting for it: the detection is queued on the detector's own
 * stream and the call returns; fm_haar_collect waits and returns its results (find_objects' detections
 * feed only the seen-objects set and the display, never the written-frame decision, fm.py:549-575, 703-731,
 * so they may be collected a batch later).  One detection in flight per detector (FM_ESTATE otherwise);
 * the frames must stay where they are until it is collected. */
int fm_haar_detect_frame_list_async(fm_haar* det, const uint8_t* const* frames, int n, int H, int W, int roi_w,
                                    double scale_factor, int min_neighbors, int* roi_h_out);
/* The results of the last detection (waits for a queued one): counts[n] (every rect) and up to cap rects
 * per image in rects[n][cap][4], as fm_haar_detect_frame_list; may be called again with a larger cap. */
int fm_haar_collect(fm_haar* det, int32_t* rects, int cap, int32_t* counts, int n);
/* The ungrouped candidates of image 0 of the last fm_haar_detect (parity
 * tests); returns their number. */
int fm_haar_candidates(const fm_haar* det, int32_t* rects, int cap);
/* Device time of the last fm_haar_detect's kernels (HIP events), ms. */
double fm_haar_last_ms(const fm_haar* det);
/* Which window sweep the last detection queued (read-only, for tests): 0 none yet or no window to
 * evaluate, 1 the tiled sweep on LDS integral patches, 2 the global-memory sweep that cascades whose
 * patches do not fit in LDS take (large or large tilted windows). */
int fm_haar_last_sweep(const fm_haar* det);

/* ---- A bank of cascades: every cascade find_objects loaded, over one frame in one pass ----
 * 1..32 cascades (members) on one device.  A call uploads and resizes the frames once, builds one
 * pyramid and one set of integral images for the longest scale list any member needs, and sweeps
 * every member's windows in one launch; each member's results are those of an fm_haar built from the
 * same description.  Min and max object sizes are the defaults (none, the image).
 * Create: every member is validated as fm_haar_create validates it, before any HIP call (FM_EINVAL,
 * the message names the member; also for n_members outside 1..32); FM_ENOTSUP for a member whose
 * window does not fit the tiled sweep's LDS patches (the ones fm_haar_last_sweep reports as 2): keep
 * a separate fm_haar for it.  *out is set even on failure, for fm_haar_bank_last_error. */
typedef struct fm_haar_bank fm_haar_bank;
int fm_haar_bank_create(int device, const fm_haar_desc* descs, int n_members, fm_haar_bank** out);
void fm_haar_bank_destroy(fm_haar_bank* bank);
const char* fm_haar_bank_last_error(const fm_haar_bank* bank);
int fm_haar_bank_size(const fm_haar_bank* bank); /* members; 0 for a bank that failed to build */
/* fm_haar_detect for every member: rects[member][image][cap][4], counts[member][image] (may exceed
 * cap; only cap are written). */
int fm_haar_bank_detect(fm_haar_bank* bank, const uint8_t* images, int n, int H, int W, int channels, int on_device,
                        double scale_factor, int min_neighbors, int32_t* rects, int cap, int32_t* counts);
/* fm_haar_detect_frames, _frame_list, _frame_list_async, fm_haar_collect and fm_haar_set_roi_upscale
 * for a bank: one INTER_AREA resize to roi_w, results laid out as fm_haar_bank_detect's.  One
 * detection in flight per bank (FM_ESTATE otherwise, and for a collect with another n); a queue that
 * failed leaves nothing to collect. */
int fm_haar_bank_set_roi_upscale(fm_haar_bank* bank, int on);
int fm_haar_bank_detect_frames(fm_haar_bank* bank, const uint8_t* frames, int n, int H, int W, int on_device,
                               int roi_w, double scale_factor, int min_neighbors, int32_t* rects, int cap,
                               int32_t* counts, int* roi_h_out);
int fm_haar_bank_detect_frame_list(fm_haar_bank* bank, const uint8_t* const* frames, int n, int H, int W, int roi_w,
                                   double scale_factor, int min_neighbors, int32_t* rects, int cap, int32_t* counts,
                                   int* roi_h_out);
int fm_haar_bank_detect_frame_list_async(fm_haar_bank* bank, const uint8_t* const* frames, int n, int H, int W,
                                         int roi_w, double scale_factor, int min_neighbors, int* roi_h_out);
int fm_haar_bank_collect(fm_haar_bank* bank, int32_t* rects, int cap, int32_t* counts, int n);
/* The ungrouped candidates of image 0 of the last detection, for one member (parity tests); returns
 * their number. */
int fm_haar_bank_candidates(const fm_haar_bank* bank, int member, int32_t* rects, int cap);
/* Device time of the last detection's kernels, gray to sweep (HIP events), ms. */
double fm_haar_bank_last_ms(const fm_haar_bank* bank);

/* ---- Decode side: MJPEG frames decoded on the GPU ------
 * Stands in for cv2.VideoCapture.read (find_motion.py:413, :497-506) on MJPEG
 * video, where every frame is one baseline JPEG, when the caller opts in (or
 * OpenCV is absent).  The decode is libjpeg-turbo's default one: jpeg_idct_islow,
 * fancy upsampling, integer YCbCr->RGB tables, BGR u8 HWC -- bit-exact to
 * cv2.imdecode and to OpenCV's built-in MJPEG reader (CAP_OPENCV_MJPEG), NOT to
 * cv2.VideoCapture's default FFmpeg backend (libavcodec IDCT + swscale), whose
 * output can differ by a few levels; that parity is unpinned here.
 * Frames without a DHT segment (AVI1 Motion-JPEG) get the T.81 Annex K tables,
 * as libjpeg-turbo's std_huff_tables installs them.
 * Supported: 8-bit baseline / extended-sequential Huffman JPEG, grayscale or
 * YCbCr with Cb, Cr at 1x1 and Y at 1x1, 2x1 or 2x2, restart intervals
 * optional (each interval is decoded by its own lane; without them one lane
 * decodes one frame).  The host only parses marker segments and copies the
 * entropy-coded bytes (stuffing and RSTn removed); Huffman decoding, IDCT,
 * upsampling and colour conversion run on the device.  Every frame of one
 * call must share frame 0's size, sampling and Huffman tables (an MJPEG
 * stream repeats them); quantization tables may differ per frame. */
typedef struct fm_mjpeg fm_mjpeg;
/* A decoder for width x height frames, up to max_frames per call.  *out is set
 * even on failure (fm_mjpeg_last_error says why); release with fm_mjpeg_destroy. */
int fm_mjpeg_create(int device, int width, int height, int max_frames, fm_mjpeg** out);
void fm_mjpeg_destroy(fm_mjpeg* dec);
const char* fm_mjpeg_last_error(const fm_mjpeg* dec);
/* Decode n JPEGs (host memory: jpegs[i], sizes[i] bytes) into [n][H][W][3] BGR
 * frames at out: device memory when out_on_device, else host memory.
 * Synchronous.  It runs on the decoder's own streams: a device `out` must not be
 * in use by work the caller queued on other streams (as for hipMemcpy). */
int fm_mjpeg_decode(fm_mjpeg* dec, const uint8_t* const* jpegs, const size_t* sizes, int n, uint8_t* out,
                    int out_on_device);
/* Device time of the last fm_mjpeg_decode's kernels (HIP events), ms. */
double fm_mjpeg_last_ms(const fm_mjpeg* dec);
/* The frame size, device and max_frames the decoder was created with. */
int fm_mjpeg_geometry(const fm_mjpeg* dec, int* width, int* height, int* device, int* max_frames);
/* fm_submit from compressed frames: n_frames x n_streams JPEGs in [t][s]
 * order, decoded by dec (created for this context's src_w x src_h) into the
 * batch's device buffer -- on the decoder's own two streams, used in turn, so one
 * batch's Huffman pass overlaps the previous batch's IDCT / colour kernels; the
 * context's input stream waits for the decode -- then processed as
 * fm_submit (frames, n_frames, on_device = 1) would.  The host buffers may be
 * reused when the call returns.  The decode does not wait for work queued earlier on the context's
 * streams: it writes the batch slot's input buffer, which is idle by construction (fm_wait
 * synchronised the slot's previous batch before the slot is handed out again) -- a waited-for-entry
 * event would serialise consecutive calls, whose Huffman pass overlaps the previous call's IDCT and
 * colour kernels.  FM_EINVAL (nothing enqueued) when dec was
 * created for another frame size or device, or for fewer than
 * n_frames x n_streams frames per call. */
int fm_submit_jpeg(fm_ctx* ctx, fm_mjpeg* dec, const uint8_t* const* jpegs, const size_t* sizes, int n_frames);
/* Tuning of the parallel Huffman decode (no reference counterpart): every entropy-coded segment is
 * cut into chunks of chunk_bits bits, one GPU lane each, and each lane speculates its entry state
 * by decoding from spec_bits bits before its chunk (default 512 / 512).  Results are identical
 * for any values; only the speed changes. */
int fm_mjpeg_tune(fm_mjpeg* dec, int chunk_bits, int spec_bits);
/* The source frame (BGR u8 [H][W][3], cap.read()'s frame.raw, fm.py:501) of (frame, stream) of the
 * last waited batch, copied to host memory: what the host needs of a batch submitted with
 * fm_submit_jpeg only for the frames it writes (fm.py:535-546) or shows.  Valid until the next
 * fm_wait; for fm_submit(on_device = 1) the caller's buffer must still hold the frames. */
int fm_read_frame(fm_ctx* ctx, int frame, int stream, uint8_t* out);
/* The device address of that same source frame, left in HBM: what find_objects (fm.py:703-731)
 * hands to fm_haar_detect_frames(on_device = 1) so an MJPEG frame decoded on the GPU reaches the
 * cascade without a round trip through host memory.  Valid until the next fm_wait. */
int fm_frame_device(fm_ctx* ctx, int frame, int stream, const uint8_t** out);

/* ---- Retained source frames: a frame kept in HBM after its batch slot is reused ----------------
 * fm_frame_device's address dies with the next fm_wait.  The drop-in's pre-motion cache (fm.py:549-601)
 * holds frames of older batches that may still be written, so the context keeps a pool of buffers of one
 * source frame each (src_h * src_w * 3 bytes) outside the batch slots; a retained frame's address goes to
 * fm_mjpeg_encode_frame_list, fm_haar_detect_frame_list, ... like any device frame.
 *
 * fm_retain_reserve: (re)sizes the pool to `frames` entries (>= 0; 0 frees it), each at a 256-byte
 * aligned address.  FM_ESTATE while an entry is in use, FM_EINVAL for a negative count, FM_ENOMEM
 * when the allocation fails (the previous pool stays as it was).  The pool counts in fm_footprint
 * and goes with fm_destroy. */
int fm_retain_reserve(fm_ctx* ctx, int frames);
/* Copies n source frames of the last waited batch, named as (frame, stream) pairs in frame_stream
 * [n][2], into free entries: the bytes fm_read_frame returns and fm_frame_device points at (after
 * fm_submit(on_device = 1) they are read from the caller's buffer, which must still hold them).
 * dev_out[i] receives the entry's device address.  One kernel launch does all n copies, and they
 * are complete when the call returns (the call synchronises the stream they ran on), so nothing
 * queued later -- the slot's next upload, a decode into it, an encoder -- needs ordering against them.
 * Everything is checked before anything is enqueued: FM_EINVAL for null arguments or a pair outside
 * the batch (the message names it); FM_ESTATE when no batch has been waited for, its slot was
 * resubmitted, or it has no source frames; FM_ENOMEM when fewer than n entries are free (nothing is
 * copied, the pool is unchanged).  n = 0 is FM_OK; a pair named twice gives two copies. */
int fm_retain_frames(fm_ctx* ctx, const int32_t* frame_stream, int n, const uint8_t** dev_out);
/* Frees n entries.  Every address is checked first: one the pool did not hand out, one already
 * released, or one named twice gives FM_EINVAL and nothing is released. */
int fm_release_frames(fm_ctx* ctx, const uint8_t* const* dev, int n);
/* One retained frame (an address fm_retain_frames gave, not yet released) copied to host memory. */
int fm_read_retained(fm_ctx* ctx, const uint8_t* dev, uint8_t* host_out);
/* Entries in use and the pool's size (either pointer may be null). */
int fm_retained_count(const fm_ctx* ctx, int* in_use, int* capacity);

/* ---- YUV input: NV12 / I420 / YUY2 / UYVY frames converted to BGR on the GPU ------------------
 * What produces video hands out YUV, not BGR: a hardware decoder leaves NV12 surfaces (pitch, chroma
 * offset) in device memory, a V4L2 camera gives YUY2 or UYVY, raw captures are I420 / NV12 / YUY2.
 * fm_submit_yuv is fm_submit for such frames: they are converted into the batch slot's BGR input
 * buffer on the context's input stream (as fm_submit_jpeg decodes into it) and the batch proceeds
 * unchanged, so 1.5 or 2 bytes per pixel cross PCIe instead of 3, and a decoder's surface needs no
 * round trip through the host.  The conversion is cv2.cvtColor(yuv, COLOR_YUV2BGR_{NV12,I420,YUY2,
 * UYVY}) as OpenCV 4.x computes it -- BT.601 limited range in 20-bit fixed point, the chroma pair of
 * a 2x1 / 2x2 group replicated:
 *   uu = U - 128, vv = V - 128, y = max(0, Y - 16) * 1220542
 *   R = sat_u8((y + 524288 + 1673527 vv) >> 20),  B = sat_u8((y + 524288 + 2116026 uu) >> 20)
 *   G = sat_u8((y + 524288 - 852492 vv - 409993 uu) >> 20)            (>> floors negative sums)
 * restated from OpenCV's source; OpenCV is not in the build image, so that parity is unpinned.
 * Layouts of one W x H frame (W even; H even for NV12 / I420):
 *   NV12  Y plane (H rows of `pitch` bytes), at chroma_offset H/2 rows of `pitch` bytes of U,V pairs
 *   I420  Y plane, at chroma_offset the U plane (H/2 rows of pitch/2 bytes), then the V plane
 *   YUY2  rows of Y0 U Y1 V per pixel pair;  UYVY  rows of U Y0 V Y1 */
#define FM_YUV_NV12 0
#define FM_YUV_I420 1
#define FM_YUV_YUY2 2
#define FM_YUV_UYVY 3
typedef struct fm_yuv_layout {
    int format;           /* FM_YUV_* */
    int pitch;            /* bytes per luma row (packed formats: per row); 0 = tight (W, or 2W) */
    int chroma_offset;    /* planar: bytes from frame start to the UV (NV12) / U (I420) plane;
                             0 = pitch*H.  I420: chroma rows are pitch/2 bytes, V follows U's H/2 rows */
    size_t frame_stride;  /* bytes between consecutive frames of the batch; 0 = tight */
} fm_yuv_layout;
/* *bytes = the extent of one width x height frame in this layout, from its first byte to the end of
 * its last chroma row (tight NV12 / I420: W*H*3/2, packed: 2*W*H): consecutive frames of a batch lie
 * frame_stride (0: this many) bytes apart.  Pure host code, no HIP call.  FM_EINVAL (*bytes = 0) for a
 * null argument, an unknown format, width or height < 1, odd width, odd height for NV12 / I420, pitch
 * below tight, odd pitch for I420, a nonzero chroma_offset below pitch*H, or a nonzero frame_stride
 * below the extent. */
int fm_yuv_frame_bytes(int width, int height, const fm_yuv_layout* layout, size_t* bytes);
/* fm_submit with YUV frames in [n_frames][n_streams] order, frame_stride apart.  Host memory
 * (on_device = 0): copied with hipMemcpyAsync on the input stream into the batch slot's YUV staging
 * (allocated on first use, one per slot, counted by fm_footprint); the buffer must stay valid until
 * fm_wait returns for the batch.  Device memory (on_device = 1): read in place, under fm_submit's
 * rules.  fm_read_frame / fm_frame_device give the converted BGR frame.  FM_EINVAL, with nothing
 * enqueued, for every case fm_yuv_frame_bytes refuses (the context's src_w x src_h is the frame
 * size: a context created with an odd width takes no YUV) and for n_frames outside [1, max_batch].
 * Under FM_FLAG_PROFILE the conversion is the kernel `yuv2bgr`. */
int fm_submit_yuv(fm_ctx* ctx, const uint8_t* frames, int n_frames, const fm_yuv_layout* layout, int on_device);
/* The same for n_frames x n_streams frames in device memory at separate addresses, frames[t * n_streams
 * + s] (host array of device pointers, as fm_haar_detect_frame_list takes them): a decoder's surfaces
 * are converted where they lie.  frame_stride is ignored.  The array may be reused when the call
 * returns; the frames stay until fm_wait. */
int fm_submit_yuv_list(fm_ctx* ctx, const uint8_t* const* frames, int n_frames, const fm_yuv_layout* layout);

/* ---- Write side: BGR frames encoded to baseline JPEG on the GPU for the MJPG writer ------------
 * Stands in for cv2.VideoWriter.write (find_motion.py:447-546, constructor default codec 'MJPG',
 * :303) when the caller opts in: the frames are encoded where they lie in HBM and only compressed
 * bytes cross PCIe.  The output is libjpeg-turbo's, byte for byte, as Pillow calls it --
 * Image.save(..., "JPEG", quality=q, subsampling=s[, restart_marker_blocks=n]): jpeg_set_quality(q,
 * force_baseline) tables, JDCT_ISLOW, the T.81 Annex K Huffman tables (not optimized), JFIF 1.01
 * APP0 -- i.e. the bytes videoio.MjpegAviWriter writes on the host.  cv2.VideoWriter's built-in
 * MJPG encoder is OpenCV's own code, not libjpeg: parity with its bytes is unpinned here, as the
 * FFmpeg decode parity is on the read side.
 * Supported: BGR u8 [H][W][3] frames (each frame contiguous) up to 65535 x 65535 and 2^20 blocks,
 * three components, subsampling in Pillow's values 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, quality 1..100,
 * restart_interval in MCUs (0 = none, at most 65535).  Not supported: grayscale output, optimized
 * Huffman tables, progressive, 12-bit. */
typedef struct fm_mjpeg_enc fm_mjpeg_enc;
/* The bytes from SOI through the SOS segment of such a file (the same for every frame of one
 * size and setting): *len = their number, copied to out when cap suffices.  Pure host code, no
 * HIP call.  FM_EINVAL for settings outside the ranges above (*len = 0) or a buffer too small. */
int fm_jpeg_header(int width, int height, int quality, int subsampling, int restart_interval, uint8_t* out, size_t cap,
                   size_t* len);
/* An encoder for width x height frames, up to max_frames per call.  Settings outside the ranges
 * above: FM_EINVAL before any HIP call.  *out is set even on failure (fm_mjpeg_enc_last_error says
 * why); release with fm_mjpeg_enc_destroy. */
int fm_mjpeg_enc_create(int device, int width, int height, int max_frames, int quality, int subsampling,
                        int restart_interval, fm_mjpeg_enc** out);
void fm_mjpeg_enc_destroy(fm_mjpeg_enc* enc);
const char* fm_mjpeg_enc_last_error(const fm_mjpeg_enc* enc);
/* Encode n frames [n][H][W][3]: host memory (copied to the device first), or device memory when
 * on_device (read in place).  Synchronous, on the encoder's own stream: device frames must be
 * complete (the caller synchronises the streams that wrote them).  The results stay on the device
 * until the next call; fm_mjpeg_enc_get fetches them. */
int fm_mjpeg_encode(fm_mjpeg_enc* enc, const uint8_t* frames, int n, int on_device);
/* fm_mjpeg_encode over n frames in device memory at n separate addresses (frames[i]: [H][W][3]
 * BGR), as fm_haar_detect_frame_list takes them: a frame from fm_frame_device is encoded where it
 * lies. */
int fm_mjpeg_encode_frame_list(fm_mjpeg_enc* enc, const uint8_t* const* frames, int n);
/* The complete JPEG (SOI .. EOI) of frame `frame` of the last call: *len = its size, copied to out
 * when cap suffices (FM_EINVAL otherwise; call again with *len bytes).  Only the entropy-coded
 * bytes are copied from the device. */
int fm_mjpeg_enc_get(fm_mjpeg_enc* enc, int frame, uint8_t* out, size_t cap, size_t* len);
/* The quantized coefficients of that frame (parity tests: what tells a DCT fault from a Huffman
 * fault): int16, blocks in scan (MCU-interleaved) order with dummy blocks included, 64 per block in
 * zigzag order.  Returns their number (cap counts coefficients; FM_EINVAL when it is smaller). */
int fm_mjpeg_enc_coefficients(fm_mjpeg_enc* enc, int frame, int16_t* out, size_t cap);
/* Device time of the last call, from its first kernel to its last (HIP events; the two host
 * round trips that size the buffers lie inside it), ms. */
double fm_mjpeg_enc_last_ms(const fm_mjpeg_enc* enc);

/* ---- YOLOv3 object stage ----------------------------------
 * Replaces cvlib.detect_common_objects(frame.resized, confidence=0.25,
 * model='yolov3[-tiny]') at find_motion.py:733-741: blobFromImage, the Darknet
 * network in f32 (convolutions as implicit GEMMs on the f32-input MFMA) and the
 * region layers' decode.  find_motion_amd/darknet.py reads the cfg and weights
 * files into this description; boxes and NMS are the caller's (a few dozen rows).
 * Independent of fm_ctx: one detector per model and device. */
#define FM_YOLO_CONV 0
#define FM_YOLO_MAXPOOL 1
#define FM_YOLO_UPSAMPLE 2
#define FM_YOLO_ROUTE 3
#define FM_YOLO_SHORTCUT 4
#define FM_YOLO_HEAD 5
#define FM_YOLO_CAND 9 /* floats per candidate: head, row, bx, by, bw, bh, obj, class, p */
typedef struct fm_yolo fm_yolo;
typedef struct fm_yolo_layer {
    int32_t kind;      /* FM_YOLO_* */
    int32_t filters;   /* conv: output channels */
    int32_t size;      /* conv: 1 or 3; maxpool: 2 */
    int32_t stride;    /* conv, maxpool: 1 or 2; upsample: 2 */
    int32_t pad;       /* conv: zero padding in pixels, 0 .. size / 2 */
    int32_t leaky;     /* conv: 1 = x > 0 ? x : 0.1f * x, 0 = linear */
    int32_t from[2];   /* route: source layers (absolute; from[1] = -1 for one); shortcut: from[0] */
    int64_t weight_ofs; /* conv: its [filters][c][size][size] block in weights, in floats */
    int64_t bias_ofs;  /* conv: its [filters] block in biases */
    int32_t n_mask;    /* head: anchors it decodes */
    int32_t anchor_ofs; /* head: its n_mask (w, h) pairs start at anchors[2 * anchor_ofs] */
} fm_yolo_layer;
typedef struct fm_yolo_desc {
    int32_t n_layers;
    const fm_yolo_layer* layers;
    const float* weights;  /* batch norm folded in (darknet.load_weights) */
    int64_t n_weights;
    const float* biases;
    int64_t n_biases;
    const float* anchors;  /* (w, h) pairs in network-input pixels, the heads' masks already applied */
    int32_t n_anchors;     /* pairs */
    int32_t channels;      /* network input channels (3 for frames) */
    int32_t net_w, net_h;  /* network input size (cvlib: 416 x 416 whatever the cfg's [net] says) */
    int32_t classes;
    int32_t max_frames;    /* frames per call the activation buffers are sized for */
    float zero_thresh;     /* class scores <= this are zeroed (OpenCV's region layer: 0.2) */
} fm_yolo_desc;

/* Validate the description (FM_EINVAL before any HIP call: a route or shortcut to a later layer, channel
 * counts or sizes that do not chain, a head whose input channels != n_mask * (classes + 5), offsets outside
 * the arrays ...), then upload the re-packed weights and allocate every layer's activations.  *out is set
 * even on failure so that fm_yolo_last_error can say why; release it with fm_yolo_destroy. */
int fm_yolo_create(int device, const fm_yolo_desc* desc, fm_yolo** out);
/* fm_yolo_create (which means FM_YOLO_F32) with the arithmetic chosen.  FM_YOLO_F16: the blob's table values,
 * the folded weights and every activation are f16 (each rounded to nearest even, results clamped to +-65504);
 * a convolution accumulates the f16 x f16 products in f32 on v_mfma_f32_32x32x16_f16 and adds bias and leaky
 * in f32; a shortcut is one f32 add; a convolution read by a head stores f32, so the decode is the same.
 * Before any HIP call: another precision is FM_EINVAL; in FM_YOLO_F16 a weight that is not finite in f16
 * (|w| >= 65520), a head that does not follow a convolution and a layer other than the head reading a head's
 * convolution are FM_ENOTSUP, the message naming the layer.  Every other fm_yolo_* call works alike in both:
 * fm_yolo_forward takes f32, fm_yolo_layer_output gives NCHW f32 (the stored halves widened). */
#define FM_YOLO_F32 0
#define FM_YOLO_F16 1
int fm_yolo_create_precision(int device, const fm_yolo_desc* desc, int precision, fm_yolo** out);
/* FM_YOLO_F32 or FM_YOLO_F16 (FM_EINVAL for NULL) */
int fm_yolo_precision(const fm_yolo* det);
void fm_yolo_destroy(fm_yolo* det);
const char* fm_yolo_last_error(const fm_yolo* det);
/* on: frames narrower than roi_w are enlarged as FM_FLAG_AREA_UPSCALE enlarges them; off (default): FM_ENOTSUP */
int fm_yolo_set_roi_upscale(fm_yolo* det, int on);
/* Layer `layer`'s output shape (-1: the network input); total candidate rows of all heads in *rows.
 * Any pointer may be NULL. */
int fm_yolo_layer_shape(const fm_yolo* det, int layer, int* c, int* h, int* w, int* rows);
/* find_objects' YOLO pass on n raw frames ([n][H][W][3] BGR; host memory, or device memory when
 * on_device): INTER_AREA to width roi_w (imutils.resize: height int(H * roi_w / W), *roi_h_out; FM_ENOTSUP
 * when W < roi_w and fm_yolo_set_roi_upscale is off), 8-bit INTER_LINEAR to the network size, the network, the decode.  cand[n][cap][9] gets
 * each frame's rows whose best class score exceeds `confidence`, sorted by (head, row); counts[n] their
 * number (may exceed cap; only cap are written).  More than max_frames: FM_EINVAL, nothing enqueued.
 * Synchronous. */
int fm_yolo_detect_frames(fm_yolo* det, const uint8_t* frames, int n, int H, int W, int on_device, int roi_w,
                          float confidence, float* cand, int cap, int32_t* counts, int* roi_h_out);
/* fm_yolo_detect_frames over n frames in device memory at n separate addresses (e.g. fm_frame_device). */
int fm_yolo_detect_frame_list(fm_yolo* det, const uint8_t* const* frames, int n, int H, int W, int roi_w,
                              float confidence, float* cand, int cap, int32_t* counts, int* roi_h_out);
/* The network alone on a caller's blob (host, [n][channels][net_h][net_w] f32): parity tests. */
int fm_yolo_forward(fm_yolo* det, const float* blob, int n);
/* The decode alone, on the head tensors the last call left: parity tests.  Results as fm_yolo_detect_frames. */
int fm_yolo_decode(fm_yolo* det, int n, float confidence, float* cand, int cap, int32_t* counts);
/* Layer `layer`'s activations of the last call ([n][c][h][w] f32 for the n frames it ran; -1: the network
 * input), copied to out: parity tests.  Returns their number (cap counts floats; FM_EINVAL when smaller). */
int fm_yolo_layer_output(fm_yolo* det, int layer, float* out, size_t cap);
/* Whether layer `layer` (a route) takes its inputs in place -- its sources wrote at channel offsets of its
 * buffer -- 1, or by the copy kernel, 0 (read-only, for tests).  In FM_YOLO_F16 (NHWC) a route is placed only
 * when its second source's channel offset is a multiple of 8. */
int fm_yolo_route_in_place(const fm_yolo* det, int layer);
/* Device time of the last call per stage (HIP events), ms: resize + blob, network, decode; returns their sum.
 * stages may be NULL. */
double fm_yolo_last_ms(const fm_yolo* det, double* stages);

#ifdef __cplusplus
}
#endif

#endif /* FIND_MOTION_AMD_H */
