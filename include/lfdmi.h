/*
 * lfdmi.h -- C-ABI of liblfdmi.so: the MI355X (gfx950) implementation of the per-frame hot
 * path of lfd.detecttrails.  Plain pointers and sizes only; loaded with ctypes.CDLL by
 * lfd_amd/_native.py (see INTEGRATION.md for the binding a maintainer of the reference adds).
 *
 * The reference has no FFI of its own: its seam is the Python call boundary of
 * lfd/detecttrails/__init__.py:69-71.  Each entry point below names the reference interface
 * it stands in for (file:line under /root/reference).
 *
 * Conventions
 *   - every function returns 0 on success, a negative lfdmi_status otherwise;
 *     lfdmi_last_error(ctx) gives the text.  HIP errors never abort the process.
 *   - images are row-major, C-contiguous, `n` images of h x w back to back.
 *   - `loc` says where caller buffers live: LFDMI_HOST (the library stages them) or
 *     LFDMI_DEVICE (hipMalloc'd / torch CUDA memory on ctx's device, used in place).
 *   - a frame must fit the ctx in BOTH dimensions (h <= max_h and w <= max_w), not only in area.
 *   - a ctx is bound to one device, is not thread-safe, and runs everything on one HIP
 *     stream (its own, or the caller's via lfdmi_set_stream).  Calls return after the
 *     stream has drained (synchronous at the ABI) -- except the `_begin` twins of
 *     lfdmi_detect_batch_raw and lfdmi_process_multiscale, which enqueue a call and return;
 *     lfdmi_end_oldest finishes it (see "calls in flight" below).
 *   - the library never retains or frees caller pointers.
 */
#ifndef LFDMI_H
#define LFDMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFDMI_VERSION 300

enum lfdmi_status {
    LFDMI_OK = 0,
    LFDMI_ERR_ARG = -1,         /* bad argument (shape, dtype, NULL) */
    LFDMI_ERR_DTYPE = -2,       /* dtype not valid for this operation (dim pass on uint8) */
    LFDMI_ERR_HIP = -3,         /* HIP runtime error; see lfdmi_last_error */
    LFDMI_ERR_UNSUPPORTED = -4, /* knob value not implemented (e.g. CHAIN_APPROX_TC89_*) */
    LFDMI_ERR_CAPACITY = -5,    /* frame larger than the ctx was created for / workspace overflow */
    LFDMI_ERR_NOLINES = -6      /* per-frame status: HoughLines returned no line although
                                   fit_minAreaRect detected (reference: TypeError, logged) */
};

/* LFDMI_HOST_PINNED (lfdmi_detect_batch / _raw only): host memory obtained from lfdmi_host_alloc -- the DMA engines read it in
 * place, without the staging copy ordinary host frames take */
enum { LFDMI_HOST = 0, LFDMI_DEVICE = 1, LFDMI_HOST_PINNED = 2 };
/* LFDMI_F32_BE (lfdmi_detect_batch_raw only; LFDMI_DEVICE frames of that type are byte-swapped IN PLACE): big-endian float32, the raw data unit of a BITPIX = -32 FITS image (what
 * fitsio hands the reference after its own byte swap, detecttrails.py:113); swapped on the device after the upload */
enum { LFDMI_U8 = 0, LFDMI_F32 = 1, LFDMI_F64 = 2, LFDMI_F32_BE = 3 };
/* numpy masking done before cv2.convertScaleAbs */
enum { LFDMI_PREP_NONE = 0, LFDMI_PREP_BRIGHT = 1, LFDMI_PREP_DIM = 2, LFDMI_PREP_BRIGHT_THEN_DIM = 3 };
/* cv2 constants re-exported by lfd/detecttrails/detecttrails.py:14-18 */
enum { LFDMI_RETR_EXTERNAL = 0, LFDMI_RETR_LIST = 1, LFDMI_RETR_CCOMP = 2, LFDMI_RETR_TREE = 3 };
enum { LFDMI_CHAIN_APPROX_NONE = 1, LFDMI_CHAIN_APPROX_SIMPLE = 2, LFDMI_CHAIN_APPROX_TC89_L1 = 3,
       LFDMI_CHAIN_APPROX_TC89_KCOS = 4 };
/* lfdmi_get_stage selectors (device images of the last process/detect call, per slot) */
/* GRAY: convertScaleAbs output; EQUALIZED: equalizeHist(gray) (1equBRIGHT / 6equDIM); ERODED: erode(equalized)
 * (7erodedDIM); EQU: the dilated image Canny and HoughLines see (2dilateBRIGHT / 8openedDIM); CANNY: the edge map;
 * BOX: box_img (3contoursBRIGHT / 9contoursDIM) -- debug dump names of processfield.py:349-378, :459-496 */
enum { LFDMI_STAGE_GRAY = 0, LFDMI_STAGE_EQU = 1, LFDMI_STAGE_CANNY = 2, LFDMI_STAGE_BOX = 3, LFDMI_STAGE_ERODED = 4,
       LFDMI_STAGE_EQUALIZED = 5 };

typedef struct lfdmi_ctx lfdmi_ctx;

/* The keys of params_bright / params_dim (detecttrails.py:202-230); key names == argument
 * names of process_field_bright/dim (processfield.py:291-293, :391-394).  Kernels are
 * row-major 0/1 masks in HOST memory. */
typedef struct {
    double lwTresh, thetaTresh, lineSetTresh, dro;
    double minAreaRectMinLen;
    double houghMethod;           /* passed to HoughLines as rho (processfield.py:370,488) */
    int32_t nlinesInSet;          /* 1..LFDMI_MAX_SET_LINES */
    int32_t contoursMode, contoursMethod;
    int32_t dilate_kh, dilate_kw;
    const uint8_t *dilateKernel;
    int32_t erode_kh, erode_kw;   /* dim only */
    const uint8_t *erodeKernel;
    double minFlux, addFlux;      /* dim only */
    /* Optional smoothing of Canny's input.  BASELINE's north_star lists a Gaussian stage inside Canny; cv2.Canny
     * (processfield.py:236) has none, so it is OFF unless gaussKernel > 0 and has no reference call site.  Odd size
     * 1..31; gaussSigma <= 0: cv2.getGaussianKernel's default for that size.  Semantics: lfdmi_gaussian_blur. */
    int32_t gaussKernel;
    double gaussSigma;
} lfdmi_params;

#define LFDMI_MAX_SET_LINES 64
#define LFDMI_MAX_MORPH_K 31

/* params_removestars (detecttrails.py:231-239) for one filter */
typedef struct {
    int32_t defaultxy, maxxy, magcount;
    double pixscale, maxmagdiff;
    double filter_cap;            /* filter_caps[filter] */
    int32_t filter_index;         /* 0..4 = u g r i z */
} lfdmi_rs_params;

/* photoObj columns read by removestars.py:96-104, padded to max_obj rows per frame */
typedef struct {
    int32_t max_obj;
    const int32_t *count;         /* [n] objects per frame */
    const float *rowc, *colc, *psfmag, *petro90; /* [n][max_obj][5] */
    const int32_t *nobserve, *ndetect;           /* [n][max_obj] */
    int32_t loc;                  /* where these arrays live */
} lfdmi_catalog;

/* one record per frame; what process_field needs to write a results row */
typedef struct {
    int32_t status;               /* 0 or a negative lfdmi_status for this frame */
    int32_t found;                /* 0 none, 1 bright pass, 2 dim pass */
    float rho, theta;             /* equhough[0][0] (processfield.py:384,502) */
    int32_t x1, y1, x2, y2;       /* dictify_hough, float32 evaluation (processfield.py:266-288) */
    int32_t n_lines_equ, n_lines_box;
    int32_t detection;            /* fit_minAreaRect's flag in the last pass that ran */
    int32_t rejected_by_theta;    /* check_theta returned True in the last pass that ran */
} lfdmi_result;

/* Workspace sizing.  Per in-flight frame the workspace holds dense 8-bit planes, bit rows and a set of
 * tables whose theoretical maxima (a checkerboard: H*(W/2+1) runs, N/2 contours, 2N contour rows, N Hough
 * chunks) are ~100 B/px, while sky frames use less than 1 % of that (tools/cap_survey.py).  A context is
 * therefore created with the capacities below (per frame; N = max_h*max_w); a frame that needs more in
 * any table is detected on the device (no table is ever indexed past its capacity), and the library
 * runs it again, alone, through a worst-case workspace it keeps for that purpose (created on first
 * use, one frame in flight), so no input can fail for lack of table space.  A field <= 0 means "the
 * theoretical maximum"; caps == NULL means the defaults of lfdmi_default_caps. */
typedef struct {
    int32_t run_cap;   /* runs per bit image (Canny candidates / background of the edge image); default N/16 */
    int32_t key_cap;   /* contours (edge components + holes); default N/256 */
    int32_t slot_cap;  /* contour rows (one (xmin,xmax) slot per row of every contour); default N/16 */
    int32_t list_cap;  /* Hough input chunks (pieces of pixel runs, <= 64 px) per image and list; default N/16 */
    int32_t peak_cap;  /* Hough local maxima per image (rounded up to a power of two); default 65536 */
    double min_rho;    /* HoughLines accumulators are sized for rho >= min_rho (theta >= pi/180); default 5;
                          a call with a finer rho runs through the worst-case workspace */
} lfdmi_caps;
void lfdmi_default_caps(int max_h, int max_w, lfdmi_caps *out);

int lfdmi_version(void);
/* max_inflight = frames processed concurrently (workspace is sized for that many, default capacities). */
int lfdmi_ctx_create(int device, int max_h, int max_w, int max_inflight, lfdmi_ctx **out);
int lfdmi_ctx_create_sized(int device, int max_h, int max_w, int max_inflight, const lfdmi_caps *caps,
                           lfdmi_ctx **out);
/* device bytes the workspace holds; frames re-run through the worst-case workspace since creation */
int64_t lfdmi_ctx_bytes(lfdmi_ctx *ctx);
int64_t lfdmi_spill_count(lfdmi_ctx *ctx);
/* What a context has had to do besides the fast path since it was created (out[0 .. n), n <= LFDMI_STAT_COUNT): none of
 * these changes a result, all of them cost time, so a caller (bench.py prints them) can tell a slow run from a busy one. */
enum {
    LFDMI_STAT_SPILLED = 0,        /* frames run again alone in the worst-case workspace (= lfdmi_spill_count) */
    LFDMI_STAT_SCAN_GIVEUPS = 1,   /* chunks in which the one-launch run scan gave up its look-back (GPU shared with other work);
                                      each switches the context to the three-launch scan for a while and reruns that chunk */
    LFDMI_STAT_GENERAL_RERUNS = 2, /* chunks run again because a frame needed the multi-workgroup run kernels while they were off */
    LFDMI_STAT_GENERAL_CHUNKS = 3, /* chunks that ran with the multi-workgroup run kernels switched on */
    LFDMI_STAT_CHUNKS = 4,         /* chunks processed by lfdmi_detect_batch / the per-pass entry points */
    LFDMI_STAT_CAP_GROWTHS = 5,    /* times the per-frame tables were enlarged after frames overflowed them */
    LFDMI_STAT_SCAN_FUSED_ON = 6,  /* 1 while the one-launch run scan is in use */
    LFDMI_STAT_COUNT = 7
};
int lfdmi_get_stats(lfdmi_ctx *ctx, int64_t *out, int n);
void lfdmi_ctx_destroy(lfdmi_ctx *ctx);
const char *lfdmi_last_error(lfdmi_ctx *ctx);
/* run on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own */
int lfdmi_set_stream(lfdmi_ctx *ctx, void *hip_stream);
int lfdmi_max_inflight(lfdmi_ctx *ctx);

/* ---- per-operator entry points (single images from processfield.py, and parity tests) ---- */

/* img[img<0]=0 / img[img<minFlux]=0; img[img>0]+=addFlux, then cv2.convertScaleAbs
 * (processfield.py:342,346 / :453-456), optionally after cv2.flip(img,0)
 * (detecttrails.py:124).  hist (n x 256 int32) may be NULL. */
int lfdmi_prep_u8(lfdmi_ctx *ctx, const void *src, int dtype, int n, int h, int w, int flip,
                  int mode, double minFlux, double addFlux, uint8_t *gray, int32_t *hist, int loc);
/* cv2.equalizeHist (processfield.py:347,457) */
int lfdmi_equalize_hist(lfdmi_ctx *ctx, const uint8_t *src, int n, int h, int w, uint8_t *dst,
                        int loc);
/* cv2.dilate / cv2.erode(img, kernel) (processfield.py:354,464,471); kernel on the host */
int lfdmi_dilate(lfdmi_ctx *ctx, const uint8_t *src, int n, int h, int w, const uint8_t *kernel,
                 int kh, int kw, uint8_t *dst, int loc);
int lfdmi_erode(lfdmi_ctx *ctx, const uint8_t *src, int n, int h, int w, const uint8_t *kernel,
                int kh, int kw, uint8_t *dst, int loc);
/* Optional Gaussian stage (no reference call site, see lfdmi_params.gaussKernel): cv2.getGaussianKernel(ksize, sigma,
 * CV_32F) applied separably in float32 (rows, then columns; BORDER_REFLECT_101; taps accumulated in order without FMA),
 * one final round-half-even + saturation.  OpenCV's own 8-bit path uses fixed-point taps since 3.4.1, so this is the
 * build's definition (oracle: lfo_gaussian_blur), not a cv2 parity claim. */
int lfdmi_gaussian_blur(lfdmi_ctx *ctx, const uint8_t *src, int n, int h, int w, int ksize, double sigma,
                        uint8_t *dst, int loc);
/* cv2.Canny(img, low, high) with aperture 3, L1 gradient (processfield.py:236) */
int lfdmi_canny(lfdmi_ctx *ctx, const uint8_t *src, int n, int h, int w, double low, double high,
                uint8_t *dst, int loc);
/* fit_minAreaRect (processfield.py:201-263): Canny(0,255) -> contours -> minAreaRect ->
 * side/elongation filter -> boxPoints -> int32 -> fillPoly.  box_img n*h*w u8 (may be NULL),
 * detection / n_boxes n x int32 (may be NULL). */
int lfdmi_fit_min_area_rect(lfdmi_ctx *ctx, const uint8_t *img, int n, int h, int w,
                            int contoursMode, int contoursMethod, double minAreaRectMinLen,
                            double lwTresh, uint8_t *box_img, int32_t *detection,
                            int32_t *n_boxes, int loc);
/* cv2.HoughLines(img, rho, theta, threshold) (processfield.py:370-371,488-489).
 * lines: n x max_lines x 2 float32 (rho, theta), sorted by votes descending;
 * n_lines: total number of lines found per image (may exceed max_lines). */
int lfdmi_hough_lines(lfdmi_ctx *ctx, const uint8_t *img, int n, int h, int w, double rho,
                      double theta, int threshold, int max_lines, float *lines, int32_t *n_lines,
                      int loc);
/* the raw (numangle+2) x (numrho+2) int32 vote accumulator of the same call */
int lfdmi_hough_accum(lfdmi_ctx *ctx, const uint8_t *img, int n, int h, int w, double rho,
                      double theta, int32_t *accum, int loc);
void lfdmi_hough_dims(int h, int w, double rho, double theta, int *numangle, int *numrho);
/* remove_stars (removestars.py:212-231) on float32 frames, in place */
int lfdmi_remove_stars(lfdmi_ctx *ctx, float *img, int n, int h, int w, const lfdmi_catalog *cat,
                       const lfdmi_rs_params *rs, int loc);

/* ---- whole passes ---- */

/* process_field_bright (processfield.py:291-388) on n images.  lines_equ / lines_box
 * (n x nlinesInSet x 2 float32, may be NULL) receive the first nlinesInSet Hough lines of
 * each set so the caller can run check_theta itself; results always filled. */
int lfdmi_process_bright(lfdmi_ctx *ctx, const void *img, int dtype, int n, int h, int w, int flip,
                         const lfdmi_params *p, lfdmi_result *results, float *lines_equ,
                         float *lines_box, int loc);
/* process_field_dim (processfield.py:391-506); after_bright = the array was already clamped
 * by the bright pass (detecttrails.py:125,129 share one array) */
int lfdmi_process_dim(lfdmi_ctx *ctx, const void *img, int dtype, int n, int h, int w, int flip,
                      int after_bright, const lfdmi_params *p, lfdmi_result *results,
                      float *lines_equ, float *lines_box, int loc);
/* One pass with HoughLines evaluated at several rho ("multi-scale Hough", BASELINE.json configs[4]; the
 * reference itself always calls the classic transform once, processfield.py:370-371,488-489): the front
 * end (mask .. fit_minAreaRect) runs once, then HoughLines(equ) / HoughLines(box_img) / check_theta for
 * every rhos[s].  results[s * n + i] is exactly what lfdmi_process_bright / _dim returns for frame i with
 * houghMethod = rhos[s] (p->houghMethod itself is ignored).  dim != 0: process_field_dim (after_bright as
 * in lfdmi_process_dim); dim == 0: process_field_bright.  1 <= n_scales <= LFDMI_MAX_SCALES. */
#define LFDMI_MAX_SCALES 4
int lfdmi_process_multiscale(lfdmi_ctx *ctx, const void *img, int dtype, int n, int h, int w, int flip,
                             int dim, int after_bright, const lfdmi_params *p, int n_scales,
                             const double *rhos, lfdmi_result *results, int loc);
/* process_field's hot part (detecttrails.py:119-131) for n float32 frames:
 * remove_stars (cat may be NULL) -> flip -> bright -> dim where bright found nothing.
 * frames are mutated by remove_stars only, as in the reference.  results: n records in HOST
 * memory. */
int lfdmi_detect_batch(lfdmi_ctx *ctx, float *frames, int n, int h, int w,
                       const lfdmi_catalog *cat, const lfdmi_rs_params *rs,
                       const lfdmi_params *bright, const lfdmi_params *dim, lfdmi_result *results,
                       int loc);
/* lfdmi_detect_batch with the frames' element type given: LFDMI_F32, or LFDMI_F32_BE for HOST / HOST_PINNED frames holding the
 * big-endian data unit of a FITS image as read from the file (DetectTrails.process reads frame files straight into pinned
 * memory and leaves the byte swap to the device: detecttrails.py:73-117 is a read + swap + copy per frame in the reference).
 * Big-endian frames are treated as a read-only input: remove_stars' squares are applied inside the library (masked as
 * the bright sweep loads the values; a frame that has to be run again alone takes its own catalogue entry) and the caller's
 * bytes -- a file's data unit -- stay as they are; LFDMI_F32 frames are blotted in place as in lfdmi_detect_batch (complete
 * when the call returns: for device-resident frames the zero fill runs on a side stream during the call).  LFDMI_F32_BE frames
 * in DEVICE memory (data units decompressed there: lfdmi_bz2_frames) are working memory of the caller's, not a file's bytes: they are
 * byte-swapped in place and then treated like any LFDMI_F32 device frames. */
int lfdmi_detect_batch_raw(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w,
                           const lfdmi_catalog *cat, const lfdmi_rs_params *rs,
                           const lfdmi_params *bright, const lfdmi_params *dim, lfdmi_result *results,
                           int loc);
/* ---- calls in flight ------------------------------------------------------------------------------------------------------
 * A synchronous call ends with a host round trip, during which the GPU idles.  lfdmi_detect_batch_begin /
 * lfdmi_process_multiscale_begin validate everything, enqueue every chunk of the call on the context's stream and return
 * without waiting on the GPU; up to LFDMI_MAX_CALLS_IN_FLIGHT calls share the context's one workspace (only the page-locked
 * areas their records are copied into are per call), and the next call's first kernel follows the previous call's last one.
 *   Ordering     calls complete in FIFO order; lfdmi_end_oldest waits for the oldest, finishes it (records written, host frames
 *                blotted) and returns its status.
 *   Equivalence  begin + lfdmi_end_oldest gives byte-identical records to the synchronous call on the same inputs and leaves
 *                the caller's frames as it does: LFDMI_F32 frames blotted by remove_stars, big-endian host frames untouched,
 *                big-endian device frames swapped in place (by begin).
 *   Lifetimes    params (structuring elements included), rs and rhos are copied by begin.  Frames, catalogue arrays and
 *                results must stay valid and untouched until the matching lfdmi_end_oldest returns.
 *   Frames       of two calls in flight must not overlap (LFDMI_ERR_ARG; two multi-scale passes, which only read, may share).
 *   loc          LFDMI_DEVICE, or LFDMI_HOST_PINNED (memory from lfdmi_host_alloc; detect only).  LFDMI_HOST: LFDMI_ERR_ARG
 *                (the runtime stages a pageable copy synchronously, so nothing would be left to overlap).
 *   Refused      with LFDMI_ERR_ARG, the calls in flight unaffected: a begin beyond LFDMI_MAX_CALLS_IN_FLIGHT; a begin while
 *                lfdmi_enable_timing is on; every other entry point that uses the workspace (lfdmi_detect_batch*,
 *                lfdmi_process_*, the operators, lfdmi_get_stage, lfdmi_get_counters, lfdmi_set_stream, lfdmi_enable_timing(1))
 *                while a call is in flight; lfdmi_end_oldest with nothing in flight.
 *   Errors       an error from begin (including one after some chunks were enqueued: lfdmi_debug_fail_chunk applies to
 *                lfdmi_detect_batch_begin too) or from lfdmi_end_oldest leaves the context usable: the failed call's work is
 *                drained and discarded.
 *   Destroy      lfdmi_ctx_destroy drains the calls in flight and frees everything (their results are not written).
 * What a synchronous call decides on the host between chunks (table growth, a rerun with the general run kernels or after the
 * run scan gave up, the worst-case spills) is decided at the end; a chunk that has to run again does so then, on a drained
 * stream.  The threaded feed of pageable host frames stays synchronous-only.  Callers detect the feature by these symbols
 * (LFDMI_VERSION is unchanged). */
#define LFDMI_MAX_CALLS_IN_FLIGHT 2
/* the non-blocking twin of lfdmi_detect_batch_raw: same arguments, same records, same side effects on the frames */
int lfdmi_detect_batch_begin(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, const lfdmi_catalog *cat,
                             const lfdmi_rs_params *rs, const lfdmi_params *bright, const lfdmi_params *dim,
                             lfdmi_result *results, int loc);
/* the non-blocking twin of lfdmi_process_multiscale (LFDMI_DEVICE images only) */
int lfdmi_process_multiscale_begin(lfdmi_ctx *ctx, const void *img, int dtype, int n, int h, int w, int flip, int dim,
                                   int after_bright, const lfdmi_params *p, int n_scales, const double *rhos,
                                   lfdmi_result *results, int loc);
/* waits for the oldest call in flight, finishes it (results written, host frames blotted), returns its status */
int lfdmi_end_oldest(lfdmi_ctx *ctx);
/* calls begun and not yet ended (0 .. LFDMI_MAX_CALLS_IN_FLIGHT) */
int lfdmi_calls_in_flight(lfdmi_ctx *ctx);
/* page-locked host memory for LFDMI_HOST_PINNED frames, placed on the NUMA node next to ctx's GPU (the allocating thread
 * is bound to the GPU's local CPUs; LFDMI_NUMA_PIN=0 in the environment disables the binding).  Free with lfdmi_host_free
 * (any live ctx of the same device, or NULL). */
int lfdmi_host_alloc(lfdmi_ctx *ctx, uint64_t bytes, void **out);
int lfdmi_host_free(lfdmi_ctx *ctx, void *p);
/* ---- FITS ingest on host threads (detecttrails.py:73-117 reads a frame with fitsio.read, removestars.py:96-104 the photoObj
 * columns) -- no GPU involved; plain files only (a .fits.bz2 is decompressed by the caller) ----
 * lfdmi_fits_read_frames: the primary-HDU data units of n files into dst (n x h x w big-endian float32 slots, e.g. memory
 * from lfdmi_host_alloc) with `threads` reader threads.  status[i]: 0 = BITPIX -32, NAXIS 2, h x w, no BSCALE / BZERO: the data
 * unit is in slot i as it is in the file; 1 = a FITS file of another kind (slot untouched: use a general reader); -1 = cannot
 * be opened; -2 = truncated / malformed.  hdr (may be NULL): the raw header of file i (80-byte cards up to its padded END
 * block) is copied to hdr + i * hdr_cap, hdr_len[i] = its full length (> hdr_cap: the copy is cut). */
int lfdmi_fits_read_frames(const char *const *paths, int n, int h, int w, void *dst, int threads, int32_t *status, char *hdr,
                           int hdr_cap, int32_t *hdr_len);
/* lfdmi_fits_read_photoobj: ROWC, COLC, PSFMAG, PETROTH90 (float32[5] per object) and NOBSERVE, NDETECT (integers) of the
 * binary table in HDU 1 of n files into the padded lfdmi_catalog arrays in host memory ([n][max_obj][5] / [n][max_obj]) and
 * count[n].  status[i]: 0 ok; 2 / 3 = ok but a float column holds a NaN / an infinity (math.ceil raises on those in
 * removestars.py:113-130: the caller makes it that frame's error); 1 = declined (more than max_obj rows, scaled columns,
 * another column layout: use a general reader); -1 cannot be opened; -2 malformed; -3 a wanted column is missing. */
int lfdmi_fits_read_photoobj(const char *const *paths, int n, int max_obj, float *rowc, float *colc, float *psfmag,
                             float *petro90, int32_t *nobserve, int32_t *ndetect, int32_t *count, int threads,
                             int32_t *status);
/* lfdmi_bz2_find_blocks: bit offsets of the block magics and the end-of-stream magic of a bzip2 file in host memory
 * (out[i] = bit offset * 2 + 1 for the end-of-stream magic; returns their number, the first `cap` stored) -- the blocks of a
 * .fits.bz2 frame are then decoded side by side (the reference pipes the file through bunzip2: detecttrails.py:81-109). */
int64_t lfdmi_bz2_find_blocks(const uint8_t *data, uint64_t n, uint64_t *out, int64_t cap);
/* ---- bzip2 on the device --------------------------------------------------------------------------------------------------
 * SDSS serves frames as frame-*.fits.bz2; the reference decompresses every one before it reads it (detecttrails.py:81-109:
 * `bunzip2` into $FITS_DUMP, then fitsio.read) at ~0.4 s per frame and core.  lfdmi_bz2_decode_batch decompresses n whole files
 * at once on the GPU (a frame is ~14 independent 900 kB blocks: Huffman / move-to-front a wave per block, inverse
 * Burrows-Wheeler transform as a list ranking, run-length layer as a scan; every block's CRC and the stream's CRC are
 * checked).  A handle owns its own stream and buffers and is independent of any lfdmi_ctx (one thread per handle).
 *   src + src_off[i], src_len[i]  file i's bytes in host memory (ordinary or page-locked);
 *   out_cap                        room per decompressed file;
 *   head, head_bytes               if head_bytes > 0: the first head_bytes of every decompressed file, side by side, in host
 *                                  memory (for parsing FITS headers; zero-filled beyond a file's end);
 *   out_len[i], status[i]          decompressed size, and 0 = decoded and checked, or why not (LFDMI_BZ2_*: the caller then
 *                                  decompresses that file on the host, which also produces the reference's error for broken
 *                                  files).  Concatenated streams (`bzip2 -c a b`, pbzip2) are one file.  Trailing bytes, randomised
 *                                  blocks of bzip2 < 0.9.5 and anything else unexpected: declined, not guessed at.
 * The decompressed files stay on the device until the handle's next lfdmi_bz2_decode_batch; lfdmi_bz2_fetch /
 * lfdmi_bz2_fetch_many copy ranges of them to host (loc LFDMI_HOST / LFDMI_HOST_PINNED) or device (LFDMI_DEVICE) memory. */
typedef struct lfdmi_bz2 lfdmi_bz2;
enum { LFDMI_BZ2_OK = 0, LFDMI_BZ2_MAGIC = 1, LFDMI_BZ2_RANDOMISED = 2, LFDMI_BZ2_HEADER = 3, LFDMI_BZ2_DATA = 4, LFDMI_BZ2_LENGTH = 5,
       LFDMI_BZ2_ORIGPTR = 6, LFDMI_BZ2_CRC = 7, LFDMI_BZ2_CYCLE = 8, LFDMI_BZ2_SIZE = 9, LFDMI_BZ2_STREAM = 10 };
int lfdmi_bz2_create(int device, lfdmi_bz2 **out);
void lfdmi_bz2_destroy(lfdmi_bz2 *z);
const char *lfdmi_bz2_last_error(lfdmi_bz2 *z);
int lfdmi_bz2_decode_batch(lfdmi_bz2 *z, const void *src, const uint64_t *src_off, const uint64_t *src_len, int n, uint64_t out_cap,
                           void *head, uint64_t head_bytes, uint64_t *out_len, int32_t *status);
int lfdmi_bz2_fetch(lfdmi_bz2 *z, int i, uint64_t off, uint64_t nbytes, void *dst, int loc);
int lfdmi_bz2_fetch_many(lfdmi_bz2 *z, int n, const int32_t *file, const uint64_t *off, const uint64_t *nbytes, void *const *dst, int loc);
/* Device memory of the handle's own (two buffers, which = 0 / 1: one chunk is decoded while the previous one is processed) to
 * gather decoded data units into -- lfdmi_bz2_fetch_many(..., LFDMI_DEVICE) -- and to hand to lfdmi_detect_batch_raw(...,
 * LFDMI_F32_BE, ..., LFDMI_DEVICE): compressed frames then cross PCIe once, compressed, and never return to the host. */
int lfdmi_bz2_frames(lfdmi_bz2 *z, int which, uint64_t bytes, void **dev);
/* optional: allocate now what a batch of n_files files / n_blocks blocks (out_cap bytes of output each, compressed_bytes in all) will
 * need, instead of inside the first lfdmi_bz2_decode_batch (tens of GB for a chunk of frames; can run beside the first reads) */
int lfdmi_bz2_reserve(lfdmi_bz2 *z, int n_files, int64_t n_blocks, uint64_t out_cap, uint64_t compressed_bytes);
/* milliseconds of the last batch: upload + magic search, Huffman / move-to-front, sort, inverse BWT walks, run-length + CRC + output */
int lfdmi_bz2_timings(lfdmi_bz2 *z, float *ms5);
/* Which calls keep the 8-bit stage images (gray, eroded, equalised+dilated: what the reference's debug PNGs show) for
 * lfdmi_get_stage.  mode -1 (default): the per-pass entry points (lfdmi_process_bright / _dim / _multiscale) do,
 * lfdmi_detect_batch does not; 0: no call does (batches through the per-pass entry points: an image per frame less to
 * write, and the dim pass may fuse its front end); 1: every call does.  The edge map and box image are always available. */
int lfdmi_set_stage_images(lfdmi_ctx *ctx, int mode);
/* copy a stage image (u8, h x w) of in-flight slot `slot` of the LAST call to dst; h, w must be the shape of
 * that call (LFDMI_ERR_ARG otherwise: dst is then too small or too large for what the workspace holds), and for the
 * 8-bit images the call must have kept them (lfdmi_set_stage_images; LFDMI_ERR_ARG otherwise) */
int lfdmi_get_stage(lfdmi_ctx *ctx, int slot, int which, int h, int w, uint8_t *dst, int loc);
/* diagnostics: the work counters of in-flight slots [slot0, slot0 + n) as left by the LAST pass
 * (LFDMI_COUNTERS int32 values per slot; order: keys, row slots, rectangles, equ list entries, box
 * list entries (pixel chunks the Hough kernels vote with), equ peaks, box peaks, overflow flag,
 * detection, tall keys, candidate words, background words, candidate runs, background runs, medium
 * keys, non-zero pixels of equ, of box_img, active 64 x 16 tiles, entries of the second (longer-chunk) Hough lists of equ / box,
 * holes the per-frame contour kernel met, holes among them it gave no key (their borders cannot pass the rectangle filter)) */
#define LFDMI_COUNTERS 22
int lfdmi_get_counters(lfdmi_ctx *ctx, int slot0, int n, int32_t *dst);
/* per-kernel timing for bench.py's roofline entry: when enabled, every kernel launch is
 * bracketed by HIP events on the launch stream; lfdmi_get_timing returns, per timing slot,
 * the summed device time (ms), the number of launches and the number of frames those launches
 * actually worked on (a dim-pass launch only works on frames the bright pass left undecided,
 * a Hough launch only on frames with a detected rectangle) since lfdmi_enable_timing(ctx, 1).
 * lfdmi_timing_slots() slots, named by lfdmi_timing_name(i) (the kernel's name).
 * lfdmi_timing_select(ctx, mask) restricts the bracketing to the slots whose bit is set in mask
 * (0: all again): the ~80 event records of a fully timed step cost ~6 % of it, a handful per step
 * do not, so bench.py times only the few largest kernels inside its timed region. */
int lfdmi_enable_timing(lfdmi_ctx *ctx, int on);
int lfdmi_timing_select(lfdmi_ctx *ctx, uint64_t mask);
int lfdmi_get_timing(lfdmi_ctx *ctx, float *ms, int32_t *launches, int64_t *units);
int lfdmi_timing_slots(void);
const char *lfdmi_timing_name(int slot);
/* developer tool (LFDMI_FRAME_PROFILE=1 in the environment when the context is created): per-phase clocks
 * (8 x int64 per slot, 10 ns ticks) of the last per-frame contour kernel launch, slots 0 .. n-1 */
int lfdmi_debug_frame_profile(lfdmi_ctx *ctx, int n, long long *dst);
/* test entry point: the tail of a pass on line sets handed in from outside -- the device's check_theta (k_finalize;
 * reference: lfd/detecttrails/processfield.py:36-150, zero fill :89-102) and the library's host-side dictify_hough
 * (processfield.py:266-288), exactly as lfdmi_detect_batch runs them on its own Hough lines.  h1 / h2: [n][kmax][2] float32
 * (rho, theta), n1 / n2: lines per set; out[i].rejected_by_theta = check_theta's True, out[i].found = which (1 / 2) when it
 * returns None, with rho / theta / x1 .. y2 filled in.  tests/test_gpu_stages.py feeds it the reference-generated vectors of
 * tests/golden/tail_fixtures.json. */
int lfdmi_debug_tail(lfdmi_ctx *ctx, int n, int kmax, const float *h1, const int32_t *n1, const float *h2, const int32_t *n2,
                     int navg, double dro, double thetaTresh, double lineSetTresh, int which, int h, int w, lfdmi_result *out);
/* developer hook for tests of the error path: the NEXT lfdmi_detect_batch call on this context returns LFDMI_ERR_ARG at the
 * top of its chunk number `chunk` (0-based; a chunk is the feed's unit for host frames, max_inflight frames otherwise),
 * after the earlier chunks ran normally; -1 disarms.  The context stays usable. */
int lfdmi_debug_fail_chunk(lfdmi_ctx *ctx, int chunk);
/* developer hooks for tests of the measurement units' chunk loops (lfdmi_light_curves, lfdmi_mask_trails, lfdmi_trail_strips,
 * lfdmi_subtract_trails, lfdmi_inject_trails, lfdmi_find_stars, lfdmi_stack_profiles).  Each of these calls goes through the
 * device in chunks of jobs, staging slots, batches of cells and launches whose sizes are compiled in and far beyond what a quick
 * test reaches.  lfdmi_debug_unit_limits lowers them for the later unit calls on this context: a field of 0 leaves that limit at
 * its compiled value, a positive field replaces it where it is smaller (a unit takes the minimum of the two, so no setting makes
 * an allocation or a launch larger than the default does), a negative field is LFDMI_ERR_ARG and changes nothing; lim == NULL
 * restores every default.  No result depends on a limit.
 *   list_pairs        (job, tile) pairs a chunk lists: a chunk holds max(1, list_pairs / tiles) jobs      (default 8 Mi)
 *   stage_bytes       bytes of host frames and host planes a chunk stages: max(1, stage_bytes / bytes per job) jobs
 *                     (512 MiB; find_stars and stack_profiles: 1 GiB, frames per chunk or group); no effect on device buffers
 *   cell_bytes        bytes of 16-byte cells: trail_strips opens a new batch of segments, subtract_trails a new chunk of frames,
 *                     when the next segment's (frame's) cells no longer fit; one segment (frame) alone always does  (512 MiB)
 *                     (frame_previews: bytes of its 8-byte cell plane, max(1, cell_bytes / (8 Hp Wp)) frames a chunk (1 GiB); its
 *                     host frames by stage_bytes (1 GiB); its chunks of frames in out[0])
 *   render_blocks     persistent blocks that walk a chunk's list: the grid is min(pairs of the chunk, render_blocks)   (2048)
 *   stars_rec_bytes   find_stars: bytes of records a chunk returns to the host: max(1, bytes / (max_obj * 32)) frames   (256 MiB)
 *                     (measure_seeing: bytes of per-record sums of a chunk: max(1, bytes / (max_obj * 64)) frames; its host
 *                     frames by stage_bytes as find_stars', its chunks of frames in out[0])
 *   stack_part_bytes  stack_profiles: bytes of block sums and counts of one launch: whole segments up to
 *                     max(1, bytes / (8 * bins)) blocks, a single segment that needs more alone                   (128 MiB)
 *                     (a segment takes (a_last >> 5) - (a_first >> 5) + 2 blocks of 32 columns, its two halves apart)
 * lfdmi_debug_unit_split writes the split of the context's last unit call to out[0 .. n-1] (entries past
 * LFDMI_UNIT_SPLIT_COUNTS are 0): out[0] chunks of jobs (find_stars: chunks of frames; stack_profiles: groups of frames),
 * out[1] batches of cells (trail_strips; 0 elsewhere), out[2] the largest grid of persistent blocks launched (0: the unit has
 * none), out[3] launches of the first pass of the first group (stack_profiles; 0 elsewhere).  A call that returns before it
 * splits anything (an error, no job) leaves zeros.  Both refuse (LFDMI_ERR_ARG) while calls are in flight.
 * The limits and the split belong to the context but are kept beside it (lfd_amd/csrc/limits/), so that this hook changes
 * nothing of the detection kernels' translation unit.  The first call of either entry with a context (lim != NULL) opens the
 * context's entry: from then on its unit calls read the limits and record their split (a struct of zeros records and lowers
 * nothing); before that, and for a context that never calls them, nothing is kept and lfdmi_debug_unit_split's first answer is
 * zeros.  lfdmi_debug_unit_limits(ctx, NULL) restores every default and closes the entry; whoever opened one calls it before
 * lfdmi_ctx_destroy, which does not know of the entry (the Python binding's Context.close does). */
typedef struct lfdmi_unit_limits {
    int64_t list_pairs, stage_bytes, cell_bytes, render_blocks, stars_rec_bytes, stack_part_bytes;
} lfdmi_unit_limits;
#define LFDMI_UNIT_SPLIT_COUNTS 4
int lfdmi_debug_unit_limits(lfdmi_ctx *ctx, const lfdmi_unit_limits *lim);
int lfdmi_debug_unit_split(lfdmi_ctx *ctx, int64_t *out, int n);
/* developer check: the device's float32 results of the three libm calls on minAreaRect's accept / reject path (angle in
 * degrees of atan2(y, x) as cv::minAreaRect rounds it; cos / sin of that angle times 0.5 as RotatedRect::points does), for
 * n host operand pairs -- compared with the host libm by tests/test_gpu_stages.py */
int lfdmi_debug_trig(lfdmi_ctx *ctx, int n, const double *y, const double *x, float *angle_deg, float *cos_half, float *sin_half);

/* ---- trail profiles ---------------------------------------------------------------------------------------------------------
 * lfdmi_measure_trails refines the Hough line of every frame whose detection record has found != 0 and measures the trail's
 * cross-section along it.  The reference defines the quantities (lfd/analysis/profiles: the observed FWHM of
 * ConvolutionObject.calc_fwhm, convolutionobj.py:160-178, and the per-cent depth of the central dip, samplers.py:158-162) but
 * measures them on no frame.  The procedure below is the definition; tests/trail_ref.py restates it in numpy and the device
 * reproduces it exactly.  Notation: R = half_width, L = seg_len, P = prof_half, K = P / prof_step (an integer).
 *
 * 1. Frame and line.  Coordinates are the detection's: x = column, y = row of the flipped frame (cv2.flip(img, 0),
 *    detecttrails.py:124), so (x, y) reads buffer row H-1-y.  The start line is x cos(th) + y sin(th) = rho with the record's
 *    float32 rho / theta widened to double; c = cos(th), s = sin(th) are taken once on the host (C library, double).  The line
 *    is then carried as a foot point f = (rho c, rho s) and a unit direction d = (-s, c); its normal is n = (d.y, -d.x).
 *    A point at position t and offset u is p = (f.x + t*d.x + u*n.x, f.y + t*d.y + u*n.y), double, evaluated left to right.
 * 2. Samples.  Bilinear in float32: x0 = floor(p.x), y0 = floor(p.y), a = (float)(p.x - x0), b = (float)(p.y - y0); with
 *    v00, v10, v01, v11 the values at (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1):
 *        top = v00 + a*(v10 - v00);  bot = v01 + a*(v11 - v01);  value = top + b*(bot - top)
 *    (float32, each operation rounded, no FMA contraction).  A sample is valid only when all four taps lie inside the frame
 *    (0 <= x0, x0+1 <= W-1, 0 <= y0, y0+1 <= H-1), are finite, and lie outside every square remove_stars zeroes for the
 *    frame's catalogue (removestars.py:212-231, the library's own k_rs_boxes geometry); so blotted LFDMI_F32 frames and
 *    unblotted LFDMI_F32_BE ones measure the same.
 *    Positions: tlo / thi are the bounds of {t : 0 <= p.x <= W-1, 0 <= p.y <= H-1} at u = 0 (per axis with d != 0: the
 *    quotients (0 - f)/d and (max - f)/d; an axis with d == 0 and f outside [0, max] leaves none); the positions are the
 *    integers t_j = tmin + j, tmin = ceil(tlo), j = 0 .. npos-1, npos = floor(thi) - tmin + 1.
 * 3. Statistic.  Every profile value m(u) is the lower median (rank floor((m-1)/2) in ascending order) of the m valid samples
 *    over the positions, at one offset u; NaN when m == 0.
 * 4. Refinement.  Passes i = 0 .. n_iter:
 *    - npos < 2L: status TOO_SHORT, stop.  Segments: j in [sL, sL+L); a last partial one is kept when it has >= L/2 positions.
 *    - per segment s, m_s(u) at integer u in [-R, R]; in double: b_s = lower median of m_s over the wings |u| > R - wing;
 *      sig_s = 1.4826 * lower median of |m_s - b_s| over the wings; A_s = max_u (m_s - b_s); s is significant when no
 *      m_s(u) is NaN, A_s > k_sig * sig_s and A_s > 0; its centre c_s = sum(u w_u) / sum(w_u), w_u = max((m_s(u) - b_s) - A_s/2, 0).
 *    - the extent is the longest run of consecutive significant segments (a tie: the first); fewer than 2 segments: status
 *      TOO_FAINT, stop.  Pass n_iter only determines the extent (on the final line).
 *    - otherwise c = a + b t is fitted by least squares weighted by A_s over the run, t = tmin + sL + (n_s - 1)/2 at the
 *      segment middles: S = sum w, St = sum w t, Stt = sum w t t, Sc = sum w c, Stc = sum w t c (in run order);
 *      b = (S Stc - St Sc) / (S Stt - St St), a = (Sc - b St) / S.  Then f += a n, d = (d + b n) / |d + b n| (sqrt of
 *      d.x d.x + d.y d.y), n from d.  All of step 4 in double, sequential in index order, no contraction.
 * 5. Result.  Over the extent's positions (j from the run's first segment start to its last segment end), m(u_k) at
 *    u_k = (k - K) * prof_step, k = 0 .. 2K (float32).  background = lower median of the non-NaN m(u_k) with |u_k| >= P - wing;
 *    the profile is v_k = m(u_k) - background (float32), peak = max of the non-NaN v_k (<= 0: TOO_FAINT).  fwhm follows
 *    calc_fwhm literally: left / right = first / last k with v_k >= peak/2, fwhm = |u_right| + |u_left|, 0 when left == right;
 *    fwhm_arcsec = fwhm * pixscale.  depth = (peak - v_K) / peak * 100 (double).  noise = 1.4826 * lower median of |v_k| over
 *    the same wing bins (double).  (x1, y1), (x2, y2) = p at the extent's first and last position (u = 0); rho / theta are
 *    the final line's (host: the normal pointing into theta in [0, pi], rho = f . n).
 * status: LFDMI_TRAIL_OK, or LFDMI_TRAIL_NOT_FOUND (record found == 0), _TOO_SHORT, _TOO_FAINT; every double of a record
 * without LFDMI_TRAIL_OK is NaN, and so is its profile row. */
typedef struct {
    int32_t half_width;  /* R: refinement window, +-R px around the line (1 .. 64); default 32 */
    int32_t seg_len;     /* L: positions per segment (2 .. 64); default 64 */
    int32_t n_iter;      /* refinement passes (0 .. 16); default 3 */
    int32_t wing;        /* wing width in px for background and noise (1 .. R); default 8 */
    double k_sig;        /* significance of a segment, in sigmas; default 5 */
    double prof_half;    /* P: profile half-width in px; default 24 */
    double prof_step;    /* profile bin step in px (P / prof_step an integer, at most 512); default 0.1: calc_fwhm takes the
                            innermost bins at or above half maximum, so it reads low by up to 2 steps (0.5 px at 0.25, 11 %
                            of a sigma = 2 px trail; 0.2 px, 4 %, at 0.1) */
    double pixscale;     /* arcsec per px; default 0.396 (SDSS) */
} lfdmi_trail_params;
enum { LFDMI_TRAIL_OK = 0, LFDMI_TRAIL_NOT_FOUND = 1, LFDMI_TRAIL_TOO_SHORT = 2, LFDMI_TRAIL_TOO_FAINT = 3 };
typedef struct {
    int32_t status;          /* LFDMI_TRAIL_* */
    int32_t n_pos;           /* positions of the extent */
    int32_t n_seg;           /* segments of the extent */
    int32_t min_valid;       /* fewest valid samples in any profile bin */
    double rho, theta;       /* the refined line (flipped frame, as the record's) */
    double x1, y1, x2, y2;   /* the extent's end points (flipped frame, as in results.txt) */
    double background, noise, peak;
    double fwhm, fwhm_arcsec, depth;
} lfdmi_trail;
void lfdmi_default_trail_params(lfdmi_trail_params *out);
/* frames: n frames of h x w, LFDMI_F32 or LFDMI_F32_BE (the bytes as they are now: big-endian device frames that
 * lfdmi_detect_batch_raw has swapped in place are LFDMI_F32 afterwards), loc LFDMI_HOST, LFDMI_HOST_PINNED or LFDMI_DEVICE;
 * rec: the n records lfdmi_detect_batch_raw returned for them (host) -- records of the FLIPPED frame (step 1); the per-pass
 * entry points give such records only with flip = 1 (records of flip = 0 calls describe the unflipped buffer and would be
 * measured along the mirrored line); cat / rs: the catalogue and remove_stars parameters
 * of that call (cat may be NULL: no squares); p NULL: the defaults; out: n records (host); profiles: n x (2K+1) float32 (host,
 * may be NULL).  The frames are only read.  Only frames with found != 0 are worked on; the workspace for it is allocated on
 * the first call. */
int lfdmi_measure_trails(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_result *rec,
                         const lfdmi_catalog *cat, const lfdmi_rs_params *rs, const lfdmi_trail_params *p, lfdmi_trail *out,
                         float *profiles);

/* ---- defocus fit ------------------------------------------------------------------------------------------------------------
 * lfdmi_fit_defocus compares the profiles of lfdmi_measure_trails with a bank of model cross-sections of a trail, built on the
 * device by lfdmi_defocus_bank_create, and reports the best model: the object's distance h, its size R and the seeing.  The
 * model is the one of lfd/analysis/profiles (Bektesevic & Vinkovic et al., arXiv 1707.07223): object (x) defocus (x) seeing,
 * plus the detector's pixel and the profile's bilinear sampling.  The reference's model functions return None in the tree
 * this follows (defocusing.py:90, seeing.py:51, objectprofiles.py:151), so the expressions in their lambdas and docstrings
 * are the definition, as below; tests/defocus_ref.py restates it in numpy.  Angles are in arcsec (RAD2ARCSEC = 206264.806247).
 *
 * 1. Components (continuous).
 *    D, defocus (defocusing.py:49-101, Eq. 6), mirrors Ro, Ri in mm, theta_o = Ro / (h 1e6), theta_i = Ri / (h 1e6) rad:
 *        D(x) = 2 / (pi (theta_o^2 - theta_i^2)) * (sqrt(theta_o^2 - x^2)_+ - [|x| < theta_i] sqrt(theta_i^2 - x^2)).
 *      (The reference's step sign(theta_i - x) is one-sided, but its nan_to_num zeroes the inner term for every |x| >
 *      theta_i, so D is symmetric.)
 *    O, object: a point (delta), or a disk of radius R m with the 1-D profile 2 sqrt(rho^2 - x^2)_+ / (pi rho^2), where
 *      rho = R / (2 h 1000) rad: the reference's angular size (objectprofiles.py:126), kept as it is (it is half the
 *      angle R / (h 1000) the disk subtends).  R = 0 is the point.
 *    S, seeing (seeing.py:29-57): sigma = 1.035 / 2.436 * FWHM; as written, both terms of 0.909 (G + 0.1 G) have the same
 *      width, so S is one Gaussian exp(-x^2 / (2 sigma^2)) normalised to unit area.  The paper may intend a wider second
 *      term; if someone pins it, it is a one-line change in k_def_kernel (and in the restatement).
 *    B, the pixel: a box 1 px wide.  T, bilinear interpolation: the triangle 1 - |x| / 1 px.  B (x) T is the phase average of
 *      measure_trails' bilinear samples.  The variance B (x) T adds along the trail's normal does not depend on the trail's
 *      angle, but its shape does: this is an approximation (the recovery test in tests/test_gpu_defocus.py measures it).
 *    The focus model (h = inf, height index n_h) has no D and a point object: S (x) B (x) T.  It is always in the bank.
 * 2. Fine grid.  delta = prof_step * pixscale / ovs arcsec; F = ovs / prof_step fine steps per px; x_j = j delta.  Every
 *    component is sampled in double at x_j and normalised to unit sum:
 *        D_j = D(x_j), |j| <= floor(theta_o / delta);  O_j = the disk at x_j, |j| <= floor(rho / delta) (point: O_0 = 1);
 *        S_j = exp(-x_j^2 / (2 sigma^2)), |j| <= floor(4 sigma / delta);
 *        B_j = max(0, min(j + 1/2, F/2) - max(j - 1/2, -F/2)) (the box's overlap with fine cell j), |j| <= ceil(F/2 - 1/2);
 *        T_j = 1 - |j| / F, |j| < F.
 *    Discrete convolutions (a (x) b)_j = sum_i a_i b_(j-i), the sum over a's support in ascending i, in double:
 *        OD = O (x) D;  KS = (S (x) B) (x) T;  M_q = sum_i OD_i KS_(q ovs - i)  (the model at bin q only).
 *    Sums of normalisation are in ascending index order.
 * 3. Columns.  The profile's bins are u_k = (k - K) prof_step px, k = 0 .. 2K (K = prof_half / prof_step).  With samp_q =
 *    M at (q - K - S) prof_step px, q = 0 .. 2K + 2S (S = max_shift), the column of shift s in [-S, S] is the model centred
 *    at s prof_step: t_k = samp_(k - s + S).  It is centred (t - mean(t), the mean over its 2K+1 bins) and scaled to unit
 *    norm in double, then rounded to float32: t^_k.  Column index ((i_seeing n_h' + i_h) n_r + i_r) (2S+1) + (s + S) with
 *    n_h' = n_h + 1 (the focus model is height index n_h; its n_r radius entries are all the point).
 * 4. Validity.  A model is invalid, and never chosen, when (theta_o + rho) / pixscale + 4 sigma / pixscale + 1 + S prof_step
 *    > prof_half - wing (px): its wings would reach the background bins of measure_trails.  An invalid model's columns are 0.
 * 5. Grid record per model (what generic_sampler(returnType="grid") reports, samplers.py:150-162): dfwhm = the FWHM of OD,
 *    ofwhm = the FWHM of samp at shift 0 (the bins u_k), both by measure_trails' calc_fwhm rule (first / last bin >= peak/2,
 *    |x_right| + |x_left|, 0 when they coincide) in arcsec; depth = (peak - samp_(K+S)) / peak * 100.  NaN for a model whose
 *    OD does not fit the profile (theta_o + rho > prof_half px); the focus model's dfwhm is 0.
 * 6. Fit of one trail.  Fitted when its record has LFDMI_TRAIL_OK, its row no NaN and noise > 0 (otherwise status
 *    LFDMI_DEFOCUS_NOT_MEASURED / _GAPS / _NO_NOISE and every double NaN).  v~ = (float)(v - mean(v)) (mean in double).
 *    Allowed columns: valid, and of the trail's seeing slice when one is given (the seeing value nearest to it; a tie: the
 *    lower).  Score c = v~ . t^, a float32 product on the matrix cores (an fmaf chain in ascending k).  The best column is
 *    the arg-max of c over the allowed columns with c > 0 (a tie: the lowest index); none: LFDMI_DEFOCUS_NO_MODEL.
 *    For it, in double, with t = samp at that shift (not normalised): a = sum (v - vbar)(t - tbar) / sum (t - tbar)^2,
 *    b = vbar - a tbar, chi2 = sum (v - a t - b)^2 / noise^2, dof = 2K - 1.
 *    chi2_by_height[i_h] = (|v~|^2 - m^2) / noise^2, m = max(0, the largest c of the allowed columns of that height) (|v~|^2
 *    in double); NaN when the height has no allowed column.  chi2_min = the least of them; h_lo / h_hi = the least / largest
 *    grid height with chi2_by_height <= chi2_min + delta_chi2 (h_hi = +inf when the focus model is among them, h_lo too when
 *    it is the only one).  The bins are correlated (about 1 / prof_step of them per px), so chi2 is a relative measure and
 *    delta_chi2 a relative threshold, not a confidence level.  The chosen model's h_km is +inf for the focus model.
 *    Degenerate rows.  A constant row has v~ = 0 and every score 0: LFDMI_DEFOCUS_NO_MODEL, chi2_by_height 0 at every height
 *    with an allowed column.  A row that holds +Inf or -Inf is not a gap: its mean is not finite, v~ holds NaN, and no score
 *    compares above 0: LFDMI_DEFOCUS_NO_MODEL, chi2_by_height NaN at every height.  Neither changes the result of any other
 *    row of the call: a row's result depends on that row, the bank and its seeing alone, not on its position or its neighbours.
 * Recovery (tests/test_gpu_defocus.py: trails rendered as the model without B and T, 8 x 8 sub-pixel points, peak 2 sky sigma,
 * ~2000 px long, three angles, then measure_trails and this fit with the default bank plus the true heights): h = 80, 100,
 * 150 km came back within 0.9 % (on the true height or the next grid height) and in-focus trails as the focus model.  The
 * interval [h_lo, h_hi] held the true height in 6 of 9 cases; in 3 (100 km at theta 0.35, 150 km at 1.2 and 2.4 rad) the fit
 * sat on the neighbouring grid height and the interval was narrower than that 0.4-0.9 % step: the median and bilinear
 * approximations bias h by more than delta_chi2 = 1 / prof_step allows.  The seeing came back within 0.13" in 8 of 9 cases
 * and 0.28" low in one (150 km at theta 2.4 rad), where defocus and seeing widen the profile alike. */
typedef struct {
    double Ro, Ri;            /* mirrors' radii in mm (SDSS 1250, 585; LSST 4180, 2558) */
    double pixscale;          /* arcsec per px: the trail params' */
    double prof_half;         /* P px: the trail params' */
    double prof_step;         /* px: the trail params' (ovs / prof_step need not be an integer) */
    int32_t wing;             /* px: the trail params' */
    int32_t ovs;              /* fine steps per profile bin (1 .. 64); default 8 */
    int32_t max_shift;        /* S: shifts of +-S bins (0 .. 64); default 5 */
    int32_t n_h, n_r, n_seeing; /* grid lengths (each >= 1; n_h <= 4096, n_r <= 64, n_seeing <= 1024; the bank's n_seeing (n_h + 1)
                                 * n_r (2S+1) columns: fewer than 2^31, and columns x padded bins x 4 bytes at most 64 GB) */
    const double *heights;    /* km, > 0, n_h of them; NULL in the defaults: 60 .. 300 km in 128 geometric steps */
    const double *radii;      /* m, >= 0; defaults {0, 0.1, 0.5, 1, 2, 5, 10} */
    const double *seeings;    /* FWHM arcsec, > 0; defaults 0.8 .. 2.2 in steps of 0.05 */
    double delta_chi2;        /* interval threshold; default 1 / prof_step */
} lfdmi_defocus_params;
typedef struct {
    double h_km;              /* +inf: the focus model */
    double radius_m, sfwhm, dfwhm, ofwhm, depth;  /* sfwhm: the seeing FWHM; dfwhm, ofwhm arcsec, depth % (step 5) */
    int32_t valid, pad;
} lfdmi_defocus_model;
enum { LFDMI_DEFOCUS_OK = 0, LFDMI_DEFOCUS_NOT_MEASURED = 1, LFDMI_DEFOCUS_GAPS = 2, LFDMI_DEFOCUS_NO_NOISE = 3,
       LFDMI_DEFOCUS_NO_MODEL = 4 };
typedef struct {
    int32_t status;           /* LFDMI_DEFOCUS_* */
    int32_t shift;            /* s of the chosen column, bins */
    int32_t dof;
    int32_t column;           /* the chosen column's index; -1 without a fit */
    double h_km, radius_m, seeing_arcsec;
    double amplitude, offset, chi2;
    double h_lo, h_hi, chi2_focus;
    double model_ofwhm, model_depth;
} lfdmi_defocus_fit;
typedef struct lfdmi_defocus_bank lfdmi_defocus_bank;
/* the defaults (SDSS mirrors and trail params, the grids above: the pointers are the library's own constant arrays) */
void lfdmi_default_defocus_params(lfdmi_defocus_params *out);
/* builds the bank on ctx's device (kept in device memory until lfdmi_defocus_bank_destroy); the grids are copied */
int lfdmi_defocus_bank_create(lfdmi_ctx *ctx, const lfdmi_defocus_params *p, lfdmi_defocus_bank **out);
/* destroy may come before or after lfdmi_ctx_destroy of the bank's context (it does not touch the context); read and fit
 * need the context alive */
void lfdmi_defocus_bank_destroy(lfdmi_defocus_bank *bank);
/* sizes of a bank: columns, models (n_seeing (n_h + 1) n_r), bins per column (2K + 1); any pointer may be NULL */
int lfdmi_defocus_bank_dims(const lfdmi_defocus_bank *bank, int64_t *n_columns, int64_t *n_models, int32_t *n_bins);
/* columns: n_columns x (2K + 1) float32 (host) or NULL; grid: n_models records (host) or NULL */
int lfdmi_defocus_bank_read(const lfdmi_defocus_bank *bank, float *columns, lfdmi_defocus_model *grid);
/* trails / profiles: n records and n x (2K + 1) float32 rows of lfdmi_measure_trails (host), with the trail params the bank
 * was built for; seeing: n FWHM values in arcsec (NaN: free) or NULL; out: n records; chi2_by_height: n x (n_h + 1) or NULL.
 * ctx must be the bank's.  The fit's workspace is allocated on the first call. */
int lfdmi_fit_defocus(lfdmi_ctx *ctx, const lfdmi_defocus_bank *bank, const lfdmi_trail *trails, const float *profiles, int n,
                      const float *seeing, lfdmi_defocus_fit *out, float *chi2_by_height);

/* ---- sky normalisation ------------------------------------------------------------------------------------------------------
 * Every other entry point assumes an SDSS frame-*.fits: sky subtracted, pixels in nanomaggies, sky sigma 0.02 - 0.05 (the
 * units minFlux / addFlux are written in).  lfdmi_sky_normalize makes a frame that still carries its sky (a pedestal, a
 * gradient, a raw exposure in ADU, an SDSS fpC file) look like that: it estimates the sky and its noise on a mesh, subtracts
 * the sky and scales the noise to target_sigma.  The reference has no such step.  The procedure below is the definition;
 * tests/sky_ref.py restates it in numpy and the device matches it bit for bit: every statistic is an exact selection, so no
 * result depends on evaluation order.  Notation: frame x of H x W float32, buffer rows (not flipped).  The lower median of m
 * values is rank floor((m-1)/2) in ascending order, as in lfdmi_measure_trails.  In the statistics a pixel -0 counts as +0.
 *
 * 1. Mesh.  ny = ceil(H / cell), nx = ceil(W / cell); cell (j, i) covers rows [j cell, min((j+1) cell, H)) and columns
 *    [i cell, min((i+1) cell, W)): the last row and column of cells may be partial.  A cell's area is its own pixel count.
 * 2. Cell statistic.  S_0 = the cell's finite pixels.  For t = 0 .. n_clip: med_t = lower median of S_t; mad_t = lower median of
 *    |v - med_t| over S_t (one float32 subtraction per element); if t < n_clip: S_(t+1) = {v in S_t : lo <= (double)v <= hi} with
 *    d = k_clip * 1.4826 * (double)mad_t, lo = (double)med_t - d, hi = (double)med_t + d (double, left to right).
 *    b = med_(n_clip), s = (float)(1.4826 * (double)mad_(n_clip)).  A cell is EMPTY when 8 |S_0| < area; its b, s are not used.
 * 3. Fill.  An empty cell takes, for b and s separately, the lower median of the non-empty cells among its up-to-8 neighbours
 *    (their step-2 values, not filled ones); without such a neighbour, the frame value of step 5.
 * 4. Filter (filter = 3; 1: none).  Each value becomes the lower median of the filled mesh over its 3 x 3 neighbourhood clipped
 *    to the mesh, written to a second mesh (never in place); the same for the s mesh.
 * 5. Frame values.  sky / sigma = lower median of b / s over the non-empty cells (step-2 values); gain = (float)(target_sigma /
 *    (double)sigma) in mode LFDMI_SKY_NORMALISE, 1 in mode LFDMI_SKY_SUBTRACT.  status: LFDMI_SKY_OK; LFDMI_SKY_NO_SKY: no
 *    non-empty cell (the output is the input with non-finite pixels set to 0; sky, sigma and the meshes are NaN, gain 1);
 *    LFDMI_SKY_NO_NOISE: NORMALISE and sigma == 0 (the sky is subtracted, gain 1).
 * 6. Background at a pixel, from the filtered b mesh m.  Cell centres cy_j = (r0 + r1 - 1) * 0.5 over the cell's own rows
 *    [r0, r1), cx_i likewise.  For row y: j = the last cell with cy_j <= y (0 when y < cy_0), j' = min(j + 1, ny - 1),
 *    ty = (float)((y - cy_j) / (cy_j' - cy_j)) (double division) when j' != j and y >= cy_j, else 0: constant outside the
 *    outermost centres.  i, i', tx likewise along the columns.  Then in float32, each operation rounded, no FMA:
 *        top = m[j][i] + tx*(m[j][i'] - m[j][i]);  bot = m[j'][i] + tx*(m[j'][i'] - m[j'][i]);  bkg = top + ty*(bot - top)
 * 7. Output.  out = (x - bkg) * gain in float32 (two rounded operations); a non-finite x gives 0.
 * Units afterwards: value = (flux - sky) * gain, so flux = value / gain + sky(pixel); trail profiles and defocus fits of a
 * normalised frame are in these units.
 * Supported range: every float32 difference v - med_t of step 2 must be finite, which pixels of magnitude up to 1.7e38 always
 * give; where one overflows, the result is not defined.  Subnormal pixels and differences are kept, never flushed to zero. */
enum { LFDMI_SKY_SUBTRACT = 0, LFDMI_SKY_NORMALISE = 1 };
enum { LFDMI_SKY_OK = 0, LFDMI_SKY_NO_SKY = 1, LFDMI_SKY_NO_NOISE = 2 };
typedef struct {
    int32_t cell;         /* mesh cell edge in px (16 .. 256); default 64 */
    int32_t n_clip;       /* clipping rounds (0 .. 8); default 3 */
    int32_t filter;       /* 3: 3 x 3 median of the mesh (default); 1: none */
    int32_t mode;         /* LFDMI_SKY_NORMALISE (default) or LFDMI_SKY_SUBTRACT */
    double k_clip;        /* clip at +- k_clip sigma (> 0); default 3 */
    double target_sigma;  /* sky sigma after NORMALISE (> 0); default 0.025: the sky sigma of lfd_amd/synth.make_frame, the recipe
                             the detection thresholds and the benchmark are quoted on */
} lfdmi_sky_params;
typedef struct {
    int32_t status;       /* LFDMI_SKY_* */
    int32_t ny, nx;       /* the mesh */
    int32_t n_empty;      /* empty cells (step 2) */
    double sky, sigma, gain;
} lfdmi_sky_frame;
typedef struct lfdmi_sky lfdmi_sky;
void lfdmi_default_sky_params(lfdmi_sky_params *out);
/* A handle for frames of exactly h x w on ctx's device: it owns the meshes, the tables of step 6, page-locked staging for host
 * frames and a device output buffer of max_frames frames.  p NULL: the defaults.  Bad arguments: LFDMI_ERR_ARG.  Destroy may
 * come before or after lfdmi_ctx_destroy of its context (it does not touch the context); normalize needs the context alive. */
int lfdmi_sky_create(lfdmi_ctx *ctx, int h, int w, int max_frames, const lfdmi_sky_params *p, lfdmi_sky **out);
void lfdmi_sky_destroy(lfdmi_sky *sky);
/* the mesh and the device bytes the handle holds; any pointer may be NULL */
int lfdmi_sky_dims(const lfdmi_sky *sky, int32_t *ny, int32_t *nx, int64_t *bytes);
/* the handle's device output buffer (max_frames x h x w float32) */
void *lfdmi_sky_frames(lfdmi_sky *sky);
/* frames: n frames, LFDMI_F32 or LFDMI_F32_BE, loc LFDMI_HOST / LFDMI_HOST_PINNED / LFDMI_DEVICE; only read (unless out == frames).
 * out (native float32, out_loc where it lives): a caller's buffer of n frames, host or device; or, for LFDMI_F32 device frames,
 * the frames themselves (in place: the statistics of a chunk are complete before any pixel of it is written); or NULL: the
 * handle's own device buffer (n <= max_frames), valid until the handle's next call and fit for lfdmi_detect_batch_raw(...,
 * LFDMI_F32, ..., LFDMI_DEVICE) and lfdmi_measure_trails.  rec: n records (host).  mesh_sky / mesh_sigma: n x ny x nx float32
 * each (host), the filtered meshes of step 4; either may be NULL.  n > max_frames runs in chunks of max_frames.  The call
 * refuses while calls are in flight (LFDMI_ERR_ARG), runs on the context's stream and waits for it once, at its end; copies
 * to pageable host memory (records, meshes, a LFDMI_HOST output) are staged by the runtime as they are queued, so the chunks
 * of a call overlap only with device or page-locked outputs. */
int lfdmi_sky_normalize(lfdmi_ctx *ctx, lfdmi_sky *sky, const void *frames, int dtype, int n, int loc, void *out, int out_loc,
                        lfdmi_sky_frame *rec, float *mesh_sky, float *mesh_sigma);

/* ---- trail injection --------------------------------------------------------------------------------------------------------
 * lfdmi_inject_trails adds model trails of known line, extent, cross-section and brightness to frames, in place: the input of
 * an efficiency measurement (inject, detect, count what comes back; lfd_amd/recovery.py).  The reference has no such step.  The
 * procedure below is the definition; tests/inject_ref.py restates it in numpy and the device reproduces it bit for bit.
 *
 * 1. Coordinates are the detection records': x = column, y = row of the flipped frame, so (x, y) is buffer row H-1-y.  A trail's
 *    line is x cos(theta) + y sin(theta) = rho, as lfdmi_result.rho / theta and lfdmi_measure_trails carry it.  c = cos(theta),
 *    s = sin(theta) are taken once on the host (C library, double); the line is a foot point f = (rho c, rho s) and a direction
 *    d = (-s, c).  The device evaluates no transcendental function.
 * 2. Tables.  n_tables rows of table_len = 2M+1 float32 (row-major); node k of a row T sits at offset (k - M) table_step px from
 *    the line: the cross-section as the sky shows it, before the pixel (the pixel integration is step 4).  T[2M+1] is read as T[2M].
 * 3. Value at a point (px, py), for a trail (table T, rho, theta, t0, t1):
 *        u = px c + py s - rho;   t = (px - f.x) d.x + (py - f.y) d.y        (double, left to right)
 *    t < t0 or t > t1: 0 (a non-finite t0 / t1 means unbounded on that side).  Otherwise q = u / table_step + M (double);
 *    q < 0 or q > 2M: 0.  Otherwise k = floor(q), a = (float)(q - k) and
 *        value = T[k] + a (T[k+1] - T[k])                                    (float32, each operation rounded, no FMA).
 * 4. Value added to pixel (x, y) by one trail: with ss = subsample and o_m = (m + 1/2) / ss - 1/2 (double), the point values at
 *    (x + o_j, y + o_i) are summed in double, i = 0 .. ss-1 the outer and j = 0 .. ss-1 the inner loop, into acc;
 *        add = (float)(amplitude acc / (ss ss))                             (double, left to right, then rounded once).
 *    add != 0: pixel = pixel + add, one float32 addition.  add == 0: the pixel is not written (its bits stay, -0 and NaN
 *    payloads included).
 * 5. Several trails on one frame are applied in ascending index order, so the result is defined bit for bit where trails cross.
 *
 * The device culls 64 x 16 pixel tiles against every trail's band (|u| <= M table_step and t in [t0, t1], widened by the
 * tile's half extent along the normal and along the line) and launches only over the surviving (frame, tile) pairs: the work
 * follows the pixels the trails reach, not the frame, and a tile without a trail causes no global write. */
#define LFDMI_INJECT_MAX_TABLE 4097   /* largest table_len (it is kept in LDS) */
typedef struct {
    int32_t frame;           /* 0 .. n-1 */
    int32_t table;           /* 0 .. n_tables-1 */
    double rho, theta;       /* the line (flipped frame); finite, |rho| <= 1e9 */
    double t0, t1;           /* extent along d from f; non-finite: unbounded on that side */
    double amplitude;        /* scale factor on the table; finite */
} lfdmi_inject_trail;
/* frames: n frames of h x w, LFDMI_F32 only (LFDMI_F32_BE is refused), loc LFDMI_DEVICE (modified in place), LFDMI_HOST or
 * LFDMI_HOST_PINNED (the frames that carry a trail are uploaded, rendered and copied back).  trails: n_trails records (host);
 * tables: n_tables x table_len float32 (host), table_len odd, 1 .. LFDMI_INJECT_MAX_TABLE; table_step > 0 px; subsample 1 .. 8.
 * Bad arguments: LFDMI_ERR_ARG, and no pixel is touched.  The call refuses while calls are in flight, runs on the context's
 * stream and waits for it once, at its end; its device memory is taken from the stream's pool and returned before that. */
int lfdmi_inject_trails(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_inject_trail *trails,
                        int n_trails, const float *tables, int n_tables, int table_len, double table_step, int subsample);

/* ---- trail masks ------------------------------------------------------------------------------------------------------------
 * lfdmi_mask_trails turns segments into pixels: every pixel of a frame whose centre lies inside a segment's band gets the
 * segment's bits in a mask plane and, optionally, a fill value in the frame.  It is what the next program asks for first:
 * photometry that skips the streak, a co-add that rejects it, a second search that must not find the same trail again.  The
 * segments are the ones every measurement ends in (lfdmi_trail.x1 .. y2 and lfdmi_stack.x1 .. y2 with their fwhm,
 * lfdmi_radon_line.ex1 .. ey2, a results row).  A pixel filled with +0 or NaN is invalid to the faint-trail search and to the
 * stacked cross-sections by their own step 1, as a pixel remove_stars blotted is, so a filled mask composes with them without a
 * new rule.  The reference has no such step.  The procedure below is the definition; tests/mask_ref.py restates it in numpy and
 * the device reproduces it byte for byte: membership is a fixed sequence of double operations and comparisons, and every other
 * result is an OR or an exact integer count, so nothing depends on the order in which the device works.
 *
 * 1. Coordinates are the detection records': x = column, y = row of the flipped frame, so pixel (x, y) is buffer row H-1-y.  The
 *    mask plane is n x h x w uint8 in buffer-row order, laid out exactly like the frames.
 * 2. Geometry of a segment (x1, y1) - (x2, y2), on the host in double, each operation rounded, no contraction:
 *        dx = x2 - x1;  dy = y2 - y1;  L = sqrt(dx*dx + dy*dy);  e = (dx / L, dy / L);  nrm = (-e.y, e.x).
 *    The segment is LFDMI_MASK_BAD_SEGMENT when an end point is not finite, a coordinate exceeds 1e6 in magnitude, L == 0,
 *    half is negative or not finite, or cap is NaN or negative.  A bad segment masks nothing and has n_pix = 0.  cap = +inf:
 *    the whole line.
 * 3. Membership of the pixel centre (x, y), x = 0 .. w-1, y = 0 .. h-1: in double, left to right, no contraction,
 *        u = ((double)x - x1) * nrm.x + ((double)y - y1) * nrm.y
 *        t = ((double)x - x1) * e.x + ((double)y - y1) * e.y
 *        inside iff fabs(u) <= half && t >= -cap && t <= L + cap            (L + cap: one addition, on the host).
 *    The device evaluates no transcendental function and no division.
 * 4. Mask.  Every inside pixel gets mask |= bits; OR does not depend on order, so crossing segments need no rule.  clear != 0:
 *    the call zeroes the n planes first; otherwise it ORs onto what the caller passed.  mask may be NULL (fill only).
 * 5. Fill (fill_mode).  LFDMI_MASK_FILL_NONE: the frames are not touched and may be NULL.  _ZERO: every pixel inside at least one
 *    segment becomes +0.0f.  _NAN: the quiet NaN 0x7fc00000.  _VALUE: (float)fill of the lowest-index segment of that frame that
 *    contains the pixel.  A pixel inside no segment is not written: its bits stay, -0 and NaN payloads included.
 * 6. Statistics, exact integers.  stats[i] = {status, n_pix}: n_pix = the pixels of the segment's frame inside segment i (a pixel
 *    two segments share counts for both); status LFDMI_MASK_OK, LFDMI_MASK_BAD_SEGMENT, or LFDMI_MASK_EMPTY for a good segment
 *    with n_pix = 0.  frame_counts[f] = the pixels of frame f inside at least one segment of this call.
 *
 * The device culls 64 x 16 pixel tiles against every segment's band (|u| <= half and t in [-cap, L + cap], widened by the tile's
 * half extent along the normal and along the line; k_mask_cull) and launches only over the surviving (frame, tile) pairs
 * (k_mask_render): a thread owns its pixels, so neither the image nor the mask sees an atomic, and a pixel inside no segment
 * causes no write.  The counts are one integer atomicAdd per wave and segment.  There is no cap on the segments of a frame. */
enum { LFDMI_MASK_OK = 0, LFDMI_MASK_BAD_SEGMENT = 1, LFDMI_MASK_EMPTY = 2 };
enum { LFDMI_MASK_FILL_NONE = 0, LFDMI_MASK_FILL_ZERO = 1, LFDMI_MASK_FILL_NAN = 2, LFDMI_MASK_FILL_VALUE = 3 };
typedef struct {
    int32_t frame;            /* 0 .. n-1 */
    uint8_t bits;             /* ORed into the mask bytes of its pixels; not 0 */
    uint8_t pad[3];
    double x1, y1, x2, y2;    /* flipped frame, as lfdmi_trail.x1 .. y2, lfdmi_radon_line.ex1 .. ey2 or a results row */
    double half;              /* half-width of the band in px (>= 0, finite) */
    double cap;               /* how far the band reaches past either end point in px (>= 0; +inf: the whole line) */
    double fill;              /* LFDMI_MASK_FILL_VALUE: the value of its pixels */
} lfdmi_mask_segment;
typedef struct {
    int32_t fill_mode;        /* LFDMI_MASK_FILL_*; default LFDMI_MASK_FILL_NONE */
    int32_t clear;            /* != 0: the mask planes are zeroed first; default 1 */
} lfdmi_mask_params;
typedef struct {
    int32_t status;           /* LFDMI_MASK_* */
    int32_t n_pix;
} lfdmi_mask_stat;
void lfdmi_default_mask_params(lfdmi_mask_params *out);
/* frames: n frames of h x w float32 at loc; needed only with a fill, which takes LFDMI_F32 and refuses LFDMI_F32_BE.  loc
 * LFDMI_DEVICE: filled in place; LFDMI_HOST / LFDMI_HOST_PINNED: the frames that carry a segment are uploaded, filled and copied
 * back, the others are neither copied nor written.  segs: n_seg records (host), any number per frame.  params NULL: the defaults.
 * mask: n x h x w uint8 at mask_loc (handled as the frames are), or NULL.  stats: n_seg records, frame_counts: n int32 (host;
 * either may be NULL).  LFDMI_ERR_ARG, and no pixel or mask byte is touched: a frame outside [0, n), bits == 0, a bad fill_mode,
 * a fill without frames, neither mask nor fill, NULL segs with n_seg > 0, h * w > 1e9.  The call keeps no state (its device memory
 * comes from the stream's pool and goes back before it returns), refuses while calls are in flight, runs on the context's
 * stream and waits for it once, at its end. */
int lfdmi_mask_trails(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_mask_segment *segs, int n_seg,
                      const lfdmi_mask_params *params, uint8_t *mask, int mask_loc, lfdmi_mask_stat *stats, int32_t *frame_counts);

/* ---- light curves -----------------------------------------------------------------------------------------------------------
 * lfdmi_light_curves measures how the brightness changes along a trail: the segment is cut into sections of sec_len px and
 * every section gets the mean of its core band above the mean of its sky bands.  Every other unit collapses the along-track
 * direction on purpose, to beat the noise; this one answers what an observer asks next: a meteor flares and fades, a tumbling
 * body glints, a trail whose rate drops to zero part-way was cut by the shutter or the chip's edge.  The segments are the ones
 * every measurement ends in, with the half-width of the trail masks.  The reference has no such step.  The procedure below is
 * the definition; tests/lc_ref.py restates it in numpy and the device reproduces it in every integer and every bit of every
 * double: a pixel enters every sum as a fixed-point integer, so the sums are integer sums and nothing depends on the order in
 * which the device works, and every double is made on the host by a fixed sequence of rounded operations.
 *
 * 1. Pixels.  Coordinates are the detection records': x = column, y = row of the flipped frame, so pixel (x, y) is buffer row
 *    H-1-y.  A pixel is valid when it is finite, not +-0 (what remove_stars or a mask fill blotted), |v| <= clip (a float32
 *    comparison) and, with a mask plane (n x h x w uint8, laid out as lfdmi_mask_trails writes it), (mask & skip_bits) == 0:
 *    this is how other trails, unblotted stars and bleed columns are kept out.  Its value enters every sum as the integer
 *        q = llrint((double)v * 1073741824.0)                              (2^30; the product is exact; ties to even).
 *    |q| <= 2^40 and a section holds fewer than 2^20 pixels at the limits below, so no int64 sum overflows.
 * 2. Geometry of a segment (x1, y1) - (x2, y2), on the host in double, each operation rounded, no contraction, exactly as step 2
 *    of the trail masks:
 *        dx = x2 - x1;  dy = y2 - y1;  L = sqrt(dx*dx + dy*dy);  e = (dx / L, dy / L);  nrm = (-e.y, e.x).
 *    The segment is LFDMI_LC_BAD_SEGMENT when an end point is not finite, a coordinate exceeds 1e6 in magnitude, L == 0, half is
 *    not finite or <= 0, bg_in or bg_out is NaN, bg_in < half, bg_out < bg_in or bg_out > LFDMI_LC_MAX_BG.
 *        inv = 1.0 / sec_len;   n_sec = max(1, (int)ceil(L * inv)).
 *    n_sec > max_sections_per_seg: LFDMI_LC_TOO_LONG.  (A results row's end points lie about 1000 px off the frame: 125 sections
 *    at the default sec_len.)
 * 3. Membership of the pixel centre (x, y), x = 0 .. w-1, y = 0 .. h-1: u and t exactly as step 3 of the trail masks,
 *        u = ((double)x - x1) * nrm.x + ((double)y - y1) * nrm.y
 *        t = ((double)x - x1) * e.x + ((double)y - y1) * e.y               (double, left to right, no contraction).
 *    The pixel takes part iff t >= 0 && t <= L; its section is j = min((int)floor(t * inv), n_sec - 1).  It is core iff
 *    fabs(u) <= half; otherwise sky iff fabs(u) >= bg_in && fabs(u) <= bg_out (both sides of the trail pooled).
 * 4. Sums, five exact integers per (segment, section): n_geom = the core pixels inside the frame, valid or not; n_core and n_sky
 *    = the valid core and sky pixels; Q_core and Q_sky = the sums of their q.  Integer addition has no order, so crossing
 *    segments, shared tiles and atomics need no rule.
 * 5. Section record j, on the host in double, each operation rounded, left to right.  t0 = j * sec_len, t1 = min((j + 1) *
 *    sec_len, L).  status LFDMI_LC_SEC_EMPTY when n_geom == 0; else LFDMI_LC_SEC_LOW when n_core < min_core or n_sky < min_sky;
 *    in both the doubles below are NaN and the integers are kept.  Else LFDMI_LC_SEC_OK and, with s_core = (double)Q_core *
 *    2^-30 and s_sky likewise, sigma = the frame's sky sigma:
 *        mean = s_core / n_core;  bkg = s_sky / n_sky;  sb = mean - bkg;  flux = sb * n_core;
 *        flux_err = sigma * sqrt(n_core + n_core * n_core / n_sky);
 *        rate = sb * (2.0 * half)        (the flux per px of trail length; invalid core pixels are taken at the section's mean);
 *        rate_err = sigma * sqrt(1.0 / n_core + 1.0 / n_sky) * (2.0 * half);
 *        coverage = n_core / n_geom.
 *    The rows j >= n_sec of a segment, and every row of a bad segment, are zero bytes.
 * 6. Segment record.  status LFDMI_LC_OK, LFDMI_LC_BAD_SEGMENT, LFDMI_LC_TOO_LONG, or LFDMI_LC_EMPTY for a good segment without
 *    an OK section.  Over the OK sections, j ascending: n_ok, first_ok, last_ok;
 *        mean_rate = (sum of n_core_j * rate_j) / (sum of n_core_j);   mean_rate_err = 1.0 / sqrt(sum of 1.0 / (rate_err_j *
 *        rate_err_j));   chi2 = sum of d * d with d = (rate_j - mean_rate) / rate_err_j;   dof = n_ok - 1;
 *        peak_section = the j of the largest rate (ties: the lowest j), peak_rate its rate;
 *        length = sum of (t1_j - t0_j);   flux = mean_rate * length;   flux_err = mean_rate_err * length.
 *    An EMPTY record keeps n_sec, has n_ok = 0, dof = -1, first_ok = last_ok = peak_section = -1 and NaN doubles; a BAD_SEGMENT or
 *    TOO_LONG record has NaN doubles and zero integers.
 * No transcendental function appears anywhere in a record (magnitudes are made in Python: lfd_amd/lightcurve.py).
 *
 * The device follows the trail masks: it culls 64 x 16 pixel tiles against every segment's outer band (|u| <= bg_out, t in
 * [0, L], widened by the tile's half extent; k_lc_cull) and runs persistent blocks over the surviving (frame, tile) pairs
 * (k_lc_render).  A thread loads its pixels once, tests them and converts them to q; the sums of a tile go through a table in
 * LDS (integer atomics, after the lanes of a wave that share a section have added up) and from there to memory with one integer
 * atomicAdd per non-zero entry.  There is no float sum and no float atomic on the device. */
#define LFDMI_LC_MAX_SECTIONS 1024     /* largest max_sections_per_seg */
#define LFDMI_LC_MAX_BG 64.0           /* largest bg_out in px */
enum { LFDMI_LC_OK = 0, LFDMI_LC_BAD_SEGMENT = 1, LFDMI_LC_TOO_LONG = 2, LFDMI_LC_EMPTY = 3 };
enum { LFDMI_LC_SEC_OK = 0, LFDMI_LC_SEC_LOW = 1, LFDMI_LC_SEC_EMPTY = 2 };
typedef struct {
    int32_t frame;            /* 0 .. n-1 */
    int32_t pad;
    double x1, y1, x2, y2;    /* flipped frame, as lfdmi_mask_segment */
    double half;              /* the core band: |u| <= half (> 0, finite) */
    double bg_in, bg_out;     /* the sky bands: bg_in <= |u| <= bg_out (half <= bg_in <= bg_out <= LFDMI_LC_MAX_BG) */
} lfdmi_lc_segment;
typedef struct {
    double sec_len;           /* section length in px (8 .. 4096); default 32 */
    float clip;               /* a pixel above clip in magnitude is invalid (finite, 0 < clip <= 1024); default 0.125 */
    int32_t min_core;         /* valid core pixels an OK section needs (>= 1); default 32 */
    int32_t min_sky;          /* and valid sky pixels (>= 1); default 32 */
} lfdmi_lc_params;
typedef struct {
    int32_t status;           /* LFDMI_LC_SEC_* */
    int32_t n_geom, n_core, n_sky;
    int64_t q_core, q_sky;    /* Q_core, Q_sky of step 4 */
    double t0, t1;            /* the section along the segment, px from (x1, y1) */
    double mean, bkg, sb, flux, flux_err, rate, rate_err, coverage;
} lfdmi_lc_section;
typedef struct {
    int32_t status;           /* LFDMI_LC_* */
    int32_t n_sec, n_ok, first_ok, last_ok, peak_section, dof;
    int32_t pad;
    double mean_rate, mean_rate_err, chi2, peak_rate, length, flux, flux_err;
} lfdmi_lc;
void lfdmi_default_lc_params(lfdmi_lc_params *out);
/* frames: n frames of h x w, LFDMI_F32 or LFDMI_F32_BE, at loc (LFDMI_HOST / LFDMI_HOST_PINNED: the frames that carry a good
 * segment are staged on the device as lfdmi_stack_profiles stages them); only read.  mask: NULL, or n x h x w uint8 at the same
 * loc; skip_bits 0 .. 255.  segs: n_seg records (host), any number per frame.  sigma: NULL (0.025 for every frame) or n positive
 * finite values.  p NULL: the defaults.  out: n_seg records; sections: n_seg x max_sections_per_seg records (host),
 * max_sections_per_seg 1 .. LFDMI_LC_MAX_SECTIONS.  LFDMI_ERR_ARG, and no output is touched: a bad dtype or loc, n or n_seg < 0,
 * h or w outside 1 .. 65536 or h * w > 1e9, a NULL argument that is needed, a bad max_sections_per_seg or skip_bits, parameters
 * out of range, a frame outside [0, n), a bad sigma.  The call keeps no state (its device memory comes from the stream's pool
 * and goes back before it returns), refuses while calls are in flight, runs on the context's stream and waits for it once. */
int lfdmi_light_curves(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const uint8_t *mask, int skip_bits,
                       const lfdmi_lc_segment *segs, int n_seg, const float *sigma, const lfdmi_lc_params *p, lfdmi_lc *out,
                       lfdmi_lc_section *sections, int max_sections_per_seg);

/* ---- trail strips -----------------------------------------------------------------------------------------------------------
 * lfdmi_trail_strips gives the band around a segment itself, straightened: a map of n_sec sections along the trail by n_off
 * offsets across it.  The stacked cross-sections keep the offsets and sum along the trail, the light curves keep the sections
 * and sum across it; a strip keeps both, which is what a person or a classifier looks at to accept a detection, what shows a
 * width or a centre that changes along the trail, and what checks the other two units: a strip summed over its offsets is a
 * light curve's integers.  The reference has no such step.  The procedure below is the definition; tests/strip_ref.py restates
 * it in numpy and the device reproduces it in every integer and every bit of every double: a pixel enters a cell as a
 * fixed-point integer, so the sums are integer sums and nothing depends on the order in which the device works, and every
 * double is made on the host by a fixed sequence of rounded operations.
 *
 * 1. Pixels: exactly step 1 of the light curves.  The frame is the flipped one; a pixel is valid when it is finite, not +-0,
 *    |v| <= clip and (mask & skip_bits) == 0; a valid pixel enters as q = llrint((double)v * 1073741824.0).
 * 2. Geometry of a segment: dx, dy, L, e, nrm exactly as step 2 of the trail masks.  On the host, in double:
 *        inv_s = 1.0 / sec_len;  inv_u = 1.0 / step;  n_sec = max(1, (int)ceil(L * inv_s));
 *        K = max(0, (int)ceil(half * inv_u - 0.5));  n_off = 2 K + 1;  kc = (double)K + 0.5.
 *    The segment is LFDMI_STRIP_BAD_SEGMENT when an end point is not finite, a coordinate exceeds 1e6 in magnitude, L == 0,
 *    half is not finite or <= 0, or n_off > LFDMI_STRIP_MAX_OFF.  It is LFDMI_STRIP_TOO_LONG when n_sec >
 *    max_sections_per_seg (at most LFDMI_STRIP_MAX_SECTIONS) or n_sec * n_off > max_cells_per_seg.
 * 3. Membership of the pixel centre (x, y): u and t exactly as step 3 of the trail masks (double, left to right, no
 *    contraction).  The pixel takes part iff t >= 0 && t <= L && fabs(u) <= half.  Its section is j = min((int)floor(t *
 *    inv_s), n_sec - 1), its offset bin b = min(max((int)floor(u * inv_u + kc), 0), 2 K).  The centre of bin b is u_b =
 *    (double)(b - K) * step.
 * 4. Cells, three exact integers per (segment, j, b): n_geom = the pixels of the frame in the cell, valid or not; n = the valid
 *    ones; q = the sum of their q.  Cell (j, b) is record j * n_off + b of the segment's row of `cells`; the records past n_sec *
 *    n_off, and every record of a segment that is not measured, are zero bytes.  Integer addition has no order, so crossing
 *    segments, shared tiles and atomics need no rule.
 * 5. Section record j, on the host in double, each operation rounded, left to right, b ascending.  t0 = j * sec_len, t1 = min((j
 *    + 1) * sec_len, L).  hw = half - wing; bin b is a wing bin iff fabs(u_b) >= hw, else a core bin.  n_geom = the sum of the
 *    cells' n_geom; n_core and n_wing = the sums of n over the core and the wing bins; Q_wing = the int64 sum of q over the wing
 *    bins.  status LFDMI_STRIP_SEC_EMPTY when n_geom == 0; else LFDMI_STRIP_SEC_LOW when n_core < min_core or n_wing < min_wing;
 *    in both the doubles below are NaN and the integers are kept.  Else LFDMI_STRIP_SEC_OK and, with sigma the frame's sky sigma:
 *        bkg = (double)Q_wing * 2^-30 / (double)n_wing;
 *        S0 = S1 = S2 = R = 0.0;  nc = 0;  for every core bin with n_b > 0, b ascending:
 *            m = (double)q_b * 2^-30 / (double)n_b;  v = m - bkg;
 *            S0 = S0 + v;  S1 = S1 + v * u_b;  S2 = S2 + v * u_b * u_b;  R = R + 1.0 / (double)n_b;  nc = nc + 1;
 *        rate = S0 * step                        (the flux per px of trail length, as the light curves' rate and the stack's flux);
 *        rate_err = sigma * step * sqrt(R + (double)nc * (double)nc / (double)n_wing);
 *        if rate >= k_mom * rate_err:  centre = S1 / S0;  d = S2 / S0 - centre * centre;  width = sqrt(d > 0.0 ? d : 0.0);
 *        else centre = width = NaN.
 *    The rows j >= n_sec of a segment, and every row of a segment that is not measured, are zero bytes.
 * 6. Segment record.  status LFDMI_STRIP_OK, LFDMI_STRIP_BAD_SEGMENT, LFDMI_STRIP_TOO_LONG, or LFDMI_STRIP_EMPTY for a good
 *    segment without an OK section; n_sec, n_off, K; n_ok = the OK sections.  Over the OK sections whose centre is finite, j
 *    ascending (n_mom of them):
 *        mean_centre = (sum of n_core_j * centre_j) / (sum of n_core_j);   mean_width = (sum of n_core_j * width_j) / (the same);
 *        max_dev = the largest fabs(centre_j - mean_centre), dev_section its j (ties: the lowest).
 *    Without such a section the three doubles are NaN and dev_section = -1.  A BAD_SEGMENT or TOO_LONG record has NaN doubles
 *    and zero integers.
 * No transcendental function but sqrt appears anywhere.  The per-cell mean (float)((double)q * 2^-30 / (double)n) is made by
 * the caller (lfd_amd/strips.py).
 *
 * The device follows the light curves: it culls 64 x 16 pixel tiles against every segment's band (|u| <= half, t in [0, L],
 * widened by the tile's half extents; k_strip_cull) and runs persistent blocks over the surviving (frame, tile) pairs
 * (k_strip_render).  A thread loads its pixels once, tests them and converts them to q; the cells of a tile go through a table
 * in LDS (integer atomics) and from there to memory with one integer atomicAdd per non-zero entry.  There is no float sum and
 * no float atomic on the device. */
#define LFDMI_STRIP_MAX_SECTIONS 1024  /* largest max_sections_per_seg */
#define LFDMI_STRIP_MAX_OFF 129        /* largest n_off */
enum { LFDMI_STRIP_OK = 0, LFDMI_STRIP_BAD_SEGMENT = 1, LFDMI_STRIP_TOO_LONG = 2, LFDMI_STRIP_EMPTY = 3 };
enum { LFDMI_STRIP_SEC_OK = 0, LFDMI_STRIP_SEC_LOW = 1, LFDMI_STRIP_SEC_EMPTY = 2 };
typedef struct {
    int32_t frame;            /* 0 .. n-1 */
    int32_t pad;
    double x1, y1, x2, y2;    /* flipped frame, as lfdmi_mask_segment */
    double half;              /* the band: |u| <= half (> 0, finite), its outermost `wing` px on either side are sky */
} lfdmi_strip_segment;
typedef struct {
    double sec_len;           /* section length in px (4 .. 4096); default 8 */
    double step;              /* offset bin in px (0.5 .. 8); default 1 */
    double wing;              /* the bins with |u_b| >= half - wing are sky (> 0, finite); default 6 */
    double k_mom;             /* centre and width need rate >= k_mom * rate_err (>= 0, finite); default 5 */
    float clip;               /* a pixel above clip in magnitude is invalid (finite, 0 < clip <= 1024); default 0.125 */
    int32_t min_core;         /* valid core pixels an OK section needs (>= 1); default 8 */
    int32_t min_wing;         /* and valid wing pixels (>= 1); default 8 */
    int32_t pad;
} lfdmi_strip_params;
typedef struct {
    int32_t n_geom, n;
    int64_t q;
} lfdmi_strip_cell;
typedef struct {
    int32_t status;           /* LFDMI_STRIP_SEC_* */
    int32_t n_geom, n_core, n_wing;
    double t0, t1;            /* the section along the segment, px from (x1, y1) */
    double bkg, rate, rate_err, centre, width;
} lfdmi_strip_section;
typedef struct {
    int32_t status;           /* LFDMI_STRIP_* */
    int32_t n_sec, n_off, K, n_ok, n_mom, dev_section;
    int32_t pad;
    double mean_centre, mean_width, max_dev;
} lfdmi_strip;
void lfdmi_default_strip_params(lfdmi_strip_params *out);
/* frames, mask, skip_bits, segs, sigma: as lfdmi_light_curves takes them.  p NULL: the defaults.  out: n_seg records;
 * sections: n_seg x max_sections_per_seg records, max_sections_per_seg 1 .. LFDMI_STRIP_MAX_SECTIONS; cells: n_seg x
 * max_cells_per_seg records, max_cells_per_seg 1 .. LFDMI_STRIP_MAX_SECTIONS * LFDMI_STRIP_MAX_OFF (all host).  LFDMI_ERR_ARG,
 * and no output is touched: a bad dtype or loc, n or n_seg < 0, h or w outside 1 .. 65536 or h * w > 1e9, a NULL argument that
 * is needed, a bad max_sections_per_seg, max_cells_per_seg or skip_bits, parameters out of range, a frame outside [0, n), a bad
 * sigma.  The call keeps no state (its device memory comes from the stream's pool and goes back before it returns; the
 * segments go through the device in batches of at most 512 MiB of cells), refuses while calls are in flight, runs on the
 * context's stream and waits for it once. */
int lfdmi_trail_strips(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const uint8_t *mask, int skip_bits,
                       const lfdmi_strip_segment *segs, int n_seg, const float *sigma, const lfdmi_strip_params *p, lfdmi_strip *out,
                       lfdmi_strip_section *sections, int max_sections_per_seg, lfdmi_strip_cell *cells, int max_cells_per_seg);

/* ---- trail subtraction ------------------------------------------------------------------------------------------------------
 * lfdmi_subtract_trails gives back the sky under a trail: it makes a smooth, star-robust model of the trail's brightness from
 * the segment's own strip (sections along the trail by offsets across it) and subtracts the model, interpolated at every pixel
 * centre, from the frame.  lfdmi_mask_trails with a fill destroys every source the trail crosses; this leaves them standing.
 * The reference has no such step.  The procedure below is the definition; tests/sub_ref.py restates it in numpy and the device
 * equals it bit for bit: everything up to the model is exact integers, so nothing depends on the order in which the device
 * works, and the only float arithmetic is the interpolation, a fixed sequence of float32 operations as in lfdmi_inject_trails
 * step 3.  The device divides integers only.
 *
 * 1. Pixels and cells: steps 1 to 4 of the trail strips, unchanged (validity with clip and the mask plane, q = llrint(v * 2^30),
 *    the geometry, the cell integers n_geom, n, q per (segment, j, b)); LFDMI_SUB_BAD_SEGMENT and LFDMI_SUB_TOO_LONG are decided
 *    exactly as the strips decide theirs, with max_sections_per_seg and max_cells_per_seg.  The cells are taken from the frames as
 *    the caller passed them, for every segment of the call, before any pixel is written.
 * 2. Section background, int64.  Bin b is a wing bin iff fabs(u_b) >= half - wing (the strips' step 5; on the host).  N_j and Q_j
 *    = the sums of n and of q over section j's wing bins.  The section is usable iff N_j >= min_wing; then B_j = Q_j / N_j (C
 *    integer division, truncating toward zero).
 * 3. Cell excess, for a usable section j and a core bin b with n_jb >= min_n: X_jb = q_jb / n_jb - B_j (truncating division).
 *    Otherwise it is absent.
 * 4. Model.  For every (j, core b): the present X_ib with i in [max(0, j - R), min(n_sec - 1, j + R)], R = smooth; c their
 *    number.  c < min_sec: M_jb = 0.  Else sorted ascending x[0 .. c-1]: c odd, M_jb = x[(c-1)/2]; c even, M_jb = x[c/2-1] +
 *    (x[c/2] - x[c/2-1]) / 2.  m_jb = (float)((double)M_jb * 2^-30): the conversion and the product are exact, the narrowing is
 *    correctly rounded.  A wing bin has m = 0, so the model tapers to zero at the first wing bin.  A section that is itself not
 *    usable (a star above clip in its wings, say) still gets a model from its neighbours: that is the point of the median.
 * 5. Value at the pixel centre (x, y): u and t as step 3 of the trail masks.  The pixel takes part iff t >= 0 && t <= L &&
 *    fabs(u) <= half and its value as passed is finite and not +-0 (a blotted pixel stays blotted; clip and the mask plane play
 *    no part here: the trail's light under a star is removed too).  In double:
 *        a = t * inv_s - 0.5;   g = u * inv_u + (double)K;
 *        j0 = clamp((int)floor(a), 0, n_sec-1);  j1 = min(j0+1, n_sec-1);  ft = (float)min(max(a - j0, 0.0), 1.0);
 *        b0 = clamp((int)floor(g), 0, 2K);       b1 = min(b0+1, 2K);       fb = (float)min(max(g - b0, 0.0), 1.0);
 *    in float32, each operation rounded, no FMA:
 *        v0 = m[j0][b0] + fb * (m[j0][b1] - m[j0][b0]);   v1 = m[j1][b0] + fb * (m[j1][b1] - m[j1][b0]);   v = v0 + ft * (v1 - v0).
 *    v != 0: pixel = pixel - v (one float32 subtraction), n_pix += 1, q_removed += llrint((double)v * 2^30).  v == 0: the pixel
 *    is not written.
 * 6. Several segments of a frame: all models come from the frames as passed (step 1); a pixel's subtractions are applied in
 *    ascending segment index, so crossings are defined bit for bit.  A thread owns its pixels; the image sees no atomic.
 * 7. Record.  status LFDMI_SUB_OK, LFDMI_SUB_BAD_SEGMENT, LFDMI_SUB_TOO_LONG, or LFDMI_SUB_EMPTY when no cell has a model
 *    (n_model == 0).  n_sec, n_off, K; n_usable = the usable sections; n_model = the core cells with c >= min_sec; n_pix = the
 *    pixels written (apply == 0: that would be); peak_section = the section of the largest m over those cells (ties: the lowest
 *    j, then the lowest b), -1 when n_model == 0; q_removed (int64); removed = (double)q_removed * 2^-30; peak = that largest m as
 *    a double, NaN when n_model == 0.  A BAD_SEGMENT or TOO_LONG segment changes no pixel; its integers are zero, its doubles NaN.
 * 8. model (may be NULL): n_seg x max_cells_per_seg float32 (host), m_jb at j * n_off + b; everything past n_sec * n_off, and
 *    every row of a segment that is not measured, is zero.
 *
 * The device makes the cells with the strips' kernels and keeps them: only the segments and the records cross the bus.
 * k_sub_model makes each segment's table (a block per run of 16 sections, its halo of R rows in LDS, the at most 17 values of a
 * median in registers); k_sub_render walks the tiles the strips' cull listed, segments through LDS in ascending index, four
 * pixels of a row per thread, the four table reads of a pixel through L2, n_pix and q_removed as one integer atomic per wave and
 * segment.  Host frames go through the device in chunks of frames: a chunk is measured, modelled and rendered while staged once. */
#define LFDMI_SUB_MAX_SMOOTH 8         /* largest smooth */
enum { LFDMI_SUB_OK = 0, LFDMI_SUB_BAD_SEGMENT = 1, LFDMI_SUB_TOO_LONG = 2, LFDMI_SUB_EMPTY = 3 };
typedef struct {
    double sec_len;           /* section length in px (4 .. 4096); default 32 */
    double step;              /* offset bin in px (0.5 .. 8); default 1 */
    double wing;              /* the bins with |u_b| >= half - wing are sky (> 0, finite); default 6 */
    float clip;               /* a pixel above clip in magnitude is invalid (finite, 0 < clip <= 1024); default 0.125 */
    int32_t smooth;           /* R, the running median's half-window in sections (0 .. LFDMI_SUB_MAX_SMOOTH); default 2 */
    int32_t min_sec;          /* present values a model cell needs (1 .. 2 R + 1); default 3 */
    int32_t min_n;            /* valid pixels a cell needs (>= 1); default 8 */
    int32_t min_wing;         /* valid wing pixels a section needs (>= 1); default 8 */
    int32_t apply;            /* 0: the model and the counts, no pixel is written; 1: subtract; default 1 */
} lfdmi_sub_params;
typedef struct {
    int32_t status;           /* LFDMI_SUB_* */
    int32_t n_sec, n_off, K, n_usable, n_model, n_pix, peak_section;
    int64_t q_removed;
    double removed, peak;
} lfdmi_sub;
void lfdmi_default_sub_params(lfdmi_sub_params *out);
/* frames: n frames of h x w at loc.  apply == 1: LFDMI_F32 only; LFDMI_DEVICE frames are changed in place; of LFDMI_HOST /
 * LFDMI_HOST_PINNED frames those that carry a good segment are uploaded, changed and copied back, the others are neither copied
 * nor written.  apply == 0: LFDMI_F32 or LFDMI_F32_BE, nothing is written.  mask, skip_bits, segs (lfdmi_strip_segment records),
 * sigma: as lfdmi_trail_strips takes them; sigma is validated and not used.  p NULL: the defaults.  out: n_seg records; model:
 * NULL or n_seg x max_cells_per_seg float32 (host).  LFDMI_ERR_ARG, and no pixel and no output is touched: what
 * lfdmi_trail_strips refuses, LFDMI_F32_BE with apply == 1, parameters out of range (min_sec > 2 smooth + 1 among them).  The
 * call keeps no state (its device memory comes from the stream's pool and goes back before it returns), refuses while calls are
 * in flight, runs on the context's stream and waits for it once. */
int lfdmi_subtract_trails(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, int loc, const uint8_t *mask, int skip_bits,
                          const lfdmi_strip_segment *segs, int n_seg, const float *sigma, const lfdmi_sub_params *p, lfdmi_sub *out,
                          float *model, int max_sections_per_seg, int max_cells_per_seg);

/* ---- faint-trail search -----------------------------------------------------------------------------------------------------
 * The detector finds a trail whose pixels survive the 8-bit conversion; lfdmi_radon_search finds one that is faint in every
 * pixel but long: it sums the frame along every line of a dyadic family (the fast Radon transform of Goetz and Druckmueller /
 * Brady) and reports the line of largest signal-to-noise.  The reference has no such step.  The procedure below is the
 * definition; tests/radon_ref.py restates it in numpy and the device matches it bit for bit: every value of the transform is
 * one float32 sum of two values of the level before, so no result depends on how the device orders or fuses the levels.
 *
 * 1. Pixels.  Coordinates are the detection records': x = column, y = row of the flipped frame, so (x, y) is buffer row H-1-y.
 *    A pixel is valid when it is finite, not +-0 (what remove_stars blotted) and |x| <= clip (above: a star, a saturated
 *    column).  v = x where valid, else +0; m = 1 where valid, else 0.
 * 2. Binning by b = bin.  Hb = ceil(H / b), Wb = ceil(W / b); V[j][i] = the float32 sum of v over rows j b .. j b + b-1 and
 *    columns i b .. i b + b-1 that exist: rows ascending, within a row columns ascending, one sequential accumulator starting
 *    at +0.  M[j][i] = the integer sum of m over the same pixels.
 * 3. Orientations q = 0 .. 3, each a working array Q of R rows and C columns (and the same of M):
 *        q = 0: Q[r][c] = V[r][c], R = Hb, C = Wb          q = 1: Q[r][c] = V[Hb-1-r][c]
 *        q = 2: Q[r][c] = V[c][r], R = Wb, C = Hb          q = 3: Q[r][c] = V[c][Wb-1-r]
 *    P = the smallest power of two >= C; columns C .. P-1 are +0.
 * 4. Transform.  F_1[c][y][0] = Q[y][c].  For strip width n = 1, 2, .. P/2, strip j and s = 0 .. 2n-1:
 *        F_2n[j][y][s] = F_n[2j][y][s>>1] + F_n[2j+1][y + ((s+1)>>1)][s>>1]          (one float32 addition)
 *    y runs over [-(P-1), R-1]; any row outside [0, R-1] of a level-1 strip reads +0.  S_q[y][s] = F_P[0][y][s]: the sum along the
 *    dyadic line that enters column 0 at row y and rises s rows over P-1 columns.  N_q[y][s]: the same recursion on M, exact
 *    in integers, at most C b b.
 * 5. Score.  A line is a candidate when N >= min_len.  Its SNR is S / (sigma * sqrtf((float)N)): a float32 square root, product
 *    and quotient, each correctly rounded.  The frame's line is the candidate of largest SNR; ties go to the lowest (q, s, y).
 * 6. Record.  status LFDMI_RADON_OK, or LFDMI_RADON_NO_LINE without a candidate (then snr = 0, found = 0, every other field 0).
 *    found = snr >= threshold (float32).  x1, y1, x2, y2, rho, theta (double, on the host): the line runs through the working
 *    points (c = 0, r = y0) and (c = P-1, r = y0 + s); these map back through the orientation to binned (i, j) -- q = 0: (c, r),
 *    1: (c, Hb-1-r), 2: (r, c), 3: (Wb-1-r, c) -- and to pixels as b i + (b-1)/2, b j + (b-1)/2 (points outside the frame are
 *    not clipped).  theta = atan2(-(x2-x1), y2-y1) folded into [0, pi), rho = x1 cos(theta) + y1 sin(theta): the line is
 *    x cos(theta) + y sin(theta) = rho, as in lfdmi_result.
 *
 * lfdmi_radon_search_lines reports several lines per frame by peeling, and where along its line each trail starts and stops.
 * The transform of a trail is a butterfly of neighbouring lines that share its pixels, so the next best entries of one
 * transform would be the same trail again: the found line's band is blotted out of the binned frame and the frame is
 * transformed again, until nothing reaches the threshold.  tests/radon_lines_ref.py restates steps 7 - 9.
 * 7. Dyadic path.  d(c; s, P) is the row offset of line (y, s) in column c: d(0; 0, 1) = 0; for c < P/2 it is d(c; s>>1, P/2),
 *    otherwise ((s+1)>>1) + d(c - P/2; s>>1, P/2) -- step 4's recursion unrolled.  The line (q, y0, s) is the cells
 *    Q[y0 + d(c)][c], c = 0 .. C-1.
 * 8. Rounds.  Round 0 is steps 1 - 6 on V_0 = V, M_0 = M; a frame's round-k record (step 6) is kept as line k.  The frame goes
 *    on to round k+1 when that record is LFDMI_RADON_OK with found = 1 and k+1 < max_lines; otherwise it stops.  With
 *    hw = ceil(peel_halfwidth / bin) cells, V_{k+1}, M_{k+1} are V_k, M_k with every cell set to +0 / 0 whose working
 *    coordinates in orientation q are (r, c), 0 <= c < C, 0 <= r < R, |r - (y0 + d(c))| <= hw (mapped to V through step 3; the
 *    band is the whole crossing, whatever step 9 finds); steps 3 - 6 then run on them.  n_lines = the number of records with
 *    found = 1: records 0 .. n_lines-1, in peel order.  If n_lines < max_lines, record n_lines is the round that stopped the
 *    frame (its best line below the threshold, or LFDMI_RADON_NO_LINE); later records are all zero.  Record 0 is bit for bit
 *    what lfdmi_radon_search returns.
 * 9. Extent, of every record with found = 1, on the arrays it was found in (before its own peel).  a_c = Q[y0 + d(c)][c]
 *    where the row exists, else +0; m_c the same on M.  pre[0] = +0, pre[c+1] = pre[c] + a_c: one sequential float32
 *    accumulator; cnt the same sum of m_c in integers.  For 0 <= c1 <= c2 <= C-1: A = pre[c2+1] - pre[c1] (one float32
 *    subtraction), N = cnt[c2+1] - cnt[c1]; the interval is a candidate when N >= min_seg and its score is
 *    A / (sigma * sqrtf((float)N)) with step 5's three roundings.  The segment is the candidate of largest score, ties to the
 *    lowest (c1, c2); min_seg <= min_len, so a found line always has one.  ex1, ey1, ex2, ey2 (double, on the host) are the
 *    working points (c1, y0 + d(c1)) and (c2, y0 + d(c2)) through step 6's mapping.  Nothing is decided on seg_snr: it is a
 *    measurement, the maximum over about C * C / 2 intervals and therefore biased upward.  The device scores each of those
 *    intervals: C * C / 2 scores per found line (C = 1024 / 745 for an SDSS frame at bin 2).
 *
 * lfdmi_radon_search_short finds a faint trail that starts and stops inside the frame.  Steps 5 and 9 score it only as part of
 * a full crossing, whose noise divides it: a trail over a fraction f of its line scores f times the full-length trail, where
 * sqrt(f) is possible.  The transform already holds the sums of shorter lines: F_L[j][y][s] of step 4 is the sum along a
 * dyadic line of strip j, L columns long, and every such level is scored here.  tests/radon_short_ref.py restates steps
 * 10 - 12.
 * 10. Short candidates.  The scored levels of orientation q are L = min_strip, 2 min_strip, .. P/2 (min_strip a power of two
 *    >= 64; an orientation with P/2 < min_strip has none; level 32 and below exist only inside the first kernel's on-chip
 *    memory and are deliberately not scored: a 32-column candidate has too few pixels to stand above the many more lines of
 *    its level).  Entry (L, q, j, y, s), 0 <= j < P/L, y in [-(L-1), R-1], 0 <= s < L, has the sum S = F_L[j][y][s] and the count
 *    N, the same recursion on M.  It is a candidate when 2 N >= L b b: at least half of the strip line's pixels are valid (one
 *    integer rule, no knob; it also keeps a strip that straddles C or the frame's edge from scoring its few pixels).  Its
 *    score is S / (sigma * sqrtf((float)N)) with step 5's three roundings.  The frame's short candidate is the one of largest
 *    score; ties go to the lowest (L, q, j, s, y).  No candidate: LFDMI_RADON_NO_LINE, as in step 6.
 *    found = snr >= short_threshold.
 * 11. Parent line.  Sp = s * (P / L), y0 = y - d(j L; Sp, P) with d of step 7: the full dyadic line (q, y0, Sp) whose path over
 *    the columns of strip j is exactly the candidate's (the high bits of a column of strip j are j L's, and below level L the
 *    slope Sp has come down to s).  d(j L; Sp, P) is exactly s j, so y0 = y - s j >= -(L-1) P / L: the parent row may be
 *    negative but never lies below -(P-1), the lowest row of step 4; rows that do not exist are +0 in steps 8 and 9.  The
 *    record's q, y0, s and x1 .. theta are the parent line's, by step 6; n_pix, sum and snr are the candidate's.
 * 12. Extent and rounds.  Step 9 runs on the parent line with min_seg, which is at most min_strip b b / 2, so a found
 *    candidate always has a segment (its own strip is one); c1 .. ey2 are that segment's.  The rounds are step 8's with the
 *    parent line: its band of peel_halfwidth is blotted, the frame transformed again, until found = 0, LFDMI_RADON_NO_LINE or
 *    max_lines.
 *    short_threshold defaults to 8.5: the noise-only 372 x 512 frames of step 5's figures peak at 4.6 - 5.81 (bin 1) and
 *    4.18 - 5.05 (bin 2) over all their levels, and 1.4 times the largest is 8.13 (the plain search keeps 8 / 5.33 = 1.5; a
 *    whole frame has 16 times the lines of these crops).
 *
 * lfdmi_radon_search_wide finds a faint trail that is wide.  A line of step 5 is one binned cell wide; a defocused meteor trail
 * is 13 px and more, so a one-cell line collects a fraction of its flux and all of the line's noise.  Lines (y, s), (y+1, s),
 * .. (y+k-1, s) of one orientation follow the same dyadic path shifted by whole rows: they share no pixel, and together they are
 * a band k cells tall whose sum and count are the sums of k neighbouring entries of the last level.  The band slides one row at
 * a time.  tests/radon_wide_ref.py restates steps 13 - 16.
 * 13. Bands.  For orientation q, B_1 = S_q and C_1 = N_q (step 4).  For k = 1, 2, 4, .. while 2k <= max_width:
 *        B_2k[y][s] = B_k[y][s] + B_k[y+k][s]          (one float32 addition; C_2k the same sum in integers)
 *    A row above R-1 reads +0 / 0.  Entry (k, q, s, y), y in [-(P-1), R-1], is the band of lines y .. y+k-1 of slope s.
 *    max_width is a power of two from 1 to 16, in binned cells.
 * 14. Score.  A band is a candidate when C_k >= k * min_len.  Its score is B_k / (sigma * sqrtf((float)C_k)) with step 5's three
 *    roundings (C_k is at most 16 * 65535 < 2^24: the conversion is exact).  The frame's band is the candidate of largest score;
 *    ties go to the lowest (k, q, s, y).  No candidate: LFDMI_RADON_NO_LINE, as in step 6.  found = snr >= wide_threshold.
 *    wide_threshold defaults to 8: the noise-only 372 x 512 frames of step 5's figures (sixteen seeds) peak, per width 1, 2, 4,
 *    8, 16, at 5.33, 5.02, 4.91, 4.88, 4.51 (bin 1) and 4.92, 4.65, 4.79, 4.34, 4.13 (bin 2): neighbouring bands of one
 *    slope share most of their pixels, so a wider band adds few independent entries, and no width raises the ceiling of
 *    width 1, which is the plain search's; its threshold of 8 (1.5 times the largest) carries over.
 * 15. Record.  width = k and y0 is the band's lowest line.  x1 .. theta are step 6's mapping of the working points
 *    (0, y0 + (k-1)/2.0) and (P-1, y0 + s + (k-1)/2.0), the band's centre line (double, on the host).
 *    width_px = (double)(k * bin) * ((double)(P-1) / sqrt((double)((P-1) (P-1) + s s))): k cells across the column axis times
 *    the cosine of the angle between the line and that axis.  n_pix, sum and snr are the band's.
 * 16. Rounds and extent.  Step 8's rounds and step 9's extent with the band in place of the line.  The peel blots the cells
 *    with y0 + d(c) - hw <= r <= y0 + d(c) + k-1 + hw.  In the extent, a_c is the value of cell (y0 + d(c), c) (+0 where the row
 *    does not exist), to which the cells of rows +1 .. +k-1 of that column are added in ascending row order, one float32
 *    addition each, +0 for a row that does not exist; m_c is the same sum in integers, so min_seg counts the band's pixels.
 *    ex1 .. ey2 are the working points (c1, y0 + d(c1) + (k-1)/2.0) and (c2, y0 + d(c2) + (k-1)/2.0): the segment's ends on
 *    the centre line.  At k = 1 both are steps 8 and 9 as written: with max_width = 1 every record's fields equal
 *    lfdmi_radon_search_lines' bit for bit (its threshold then is wide_threshold). */
enum { LFDMI_RADON_OK = 0, LFDMI_RADON_NO_LINE = 1 };
#define LFDMI_RADON_MAX_LINES 8
typedef struct {
    int32_t bin;          /* 1, 2 or 4; default 2 */
    int32_t min_len;      /* valid pixels a candidate line needs (>= 1); default 256 */
    float clip;           /* pixels above it in magnitude are not summed (> 0); default 0.125 = five sky sigma */
    float threshold;      /* found = snr >= threshold; default 8: noise-only frames of 372 x 512 peak at 4.5 - 5.3 (bin 1), 4.2 - 4.9 (bin 2) */
} lfdmi_radon_params;
typedef struct {
    int32_t status;       /* LFDMI_RADON_* */
    int32_t found;
    int32_t q, y0, s;     /* the line in working coordinates (steps 3, 4) */
    int32_t n_pix;        /* N: valid pixels on it */
    float sum, snr;       /* S and its score */
    double x1, y1, x2, y2, rho, theta;
} lfdmi_radon_result;
typedef struct lfdmi_radon lfdmi_radon;
void lfdmi_default_radon_params(lfdmi_radon_params *out);
/* A handle for frames of exactly h x w on ctx's device: it owns V, M, two sets of planes ((R + P - 1) x P float32 sums and
 * 16-bit counts per orientation) for max_frames frames and, once host frames have been given, an upload buffer.  p NULL: the
 * defaults.  LFDMI_ERR_ARG: h or w below 2 bin, a line that could count more than 65535 pixels (max(Hb, Wb) b b: a line crosses every column of its orientation), parameters
 * out of range.  Destroy may come before or after lfdmi_ctx_destroy of its context (it does not touch the context). */
int lfdmi_radon_create(lfdmi_ctx *ctx, int h, int w, int max_frames, const lfdmi_radon_params *p, lfdmi_radon **out);
void lfdmi_radon_destroy(lfdmi_radon *radon);
/* P of orientations 0, 1 (p01) and 2, 3 (p23) and the device bytes the handle holds; any pointer may be NULL */
int lfdmi_radon_dims(const lfdmi_radon *radon, int32_t *p01, int32_t *p23, int64_t *bytes);
/* frames: n frames, LFDMI_F32 or LFDMI_F32_BE, loc LFDMI_HOST / LFDMI_HOST_PINNED / LFDMI_DEVICE; only read.  sigma: n float32
 * (host), the sky sigma of each frame, > 0; NULL: 0.025 for every frame.  results: n records (host).  n > max_frames runs in
 * chunks of max_frames.  The call refuses (LFDMI_ERR_ARG) while calls are in flight and on a sigma that is not positive, runs
 * on the context's stream and waits for it once, at its end. */
int lfdmi_radon_search(lfdmi_ctx *ctx, lfdmi_radon *radon, const void *frames, int dtype, int n, int loc, const float *sigma,
                       lfdmi_radon_result *results);
typedef struct {
    int32_t max_lines;        /* lines reported per frame at most, 1 .. LFDMI_RADON_MAX_LINES; default 4 */
    int32_t peel_halfwidth;   /* half-width in pixels of the band blotted around a found line (>= 0); default 8 */
    int32_t min_seg;          /* valid pixels a segment needs, 1 .. the handle's min_len; default 64 */
} lfdmi_radon_lines_params;
typedef struct {
    int32_t status;       /* as in lfdmi_radon_result, down to theta */
    int32_t found;
    int32_t q, y0, s;
    int32_t n_pix;
    float sum, snr;
    double x1, y1, x2, y2, rho, theta;
    int32_t c1, c2;       /* the segment: working columns c1 .. c2 of the line (step 9); found = 0: this and the rest are 0 */
    int32_t seg_n_pix;    /* N of the segment */
    int32_t pad;
    float seg_sum, seg_snr;   /* A and its score: a maximum over about C * C / 2 intervals, biased upward; nothing is decided on it */
    double ex1, ey1, ex2, ey2;   /* the segment's end points, in the coordinates of x1 .. y2 */
} lfdmi_radon_line;
void lfdmi_default_radon_lines_params(lfdmi_radon_lines_params *out);
/* lfdmi_radon_search with steps 7 - 9: frames, dtype, n, loc and sigma as there.  lp NULL: the defaults.  lines: n * max_lines
 * records (host), frame i's at lines[i * max_lines ..]; n_lines: n counts (host).  Out-of-range parameters (min_seg above the
 * handle's min_len among them): LFDMI_ERR_ARG, and nothing runs.  On its first call the handle allocates a second V, M set
 * (6 bytes per binned pixel per frame) and the lines' prefix arrays; lfdmi_radon_dims counts them from then on.  The frames
 * are only read; the call refuses while calls are in flight, runs on the context's stream and waits for it once per round
 * of each chunk (the host decides which frames continue). */
int lfdmi_radon_search_lines(lfdmi_ctx *ctx, lfdmi_radon *radon, const void *frames, int dtype, int n, int loc, const float *sigma,
                             const lfdmi_radon_lines_params *lp, lfdmi_radon_line *lines, int32_t *n_lines);
typedef struct {
    int32_t min_strip;        /* the shortest scored strip width L: a power of two >= 64; default 64 */
    int32_t max_lines;        /* records per frame at most, 1 .. LFDMI_RADON_MAX_LINES; default 4 */
    int32_t peel_halfwidth;   /* half-width in pixels of the band blotted around a found candidate's parent line (>= 0); default 8 */
    int32_t min_seg;          /* valid pixels a segment needs, 1 .. min_strip * bin * bin / 2; default 32 */
    float short_threshold;    /* found = snr >= short_threshold; finite and > 0; default 8.5 (step 12) */
    int32_t pad;
} lfdmi_radon_short_params;
typedef struct {
    int32_t status;       /* as in lfdmi_radon_line, down to ey2: q, y0, s and x1 .. theta are the parent line (step 11), */
    int32_t found;        /* n_pix, sum and snr the candidate's, found = snr >= short_threshold */
    int32_t q, y0, s;
    int32_t n_pix;
    float sum, snr;
    double x1, y1, x2, y2, rho, theta;
    int32_t c1, c2;
    int32_t seg_n_pix;
    int32_t pad;
    float seg_sum, seg_snr;
    double ex1, ey1, ex2, ey2;
    int32_t level, strip, ys, ss;   /* the candidate (step 10): L, j, y, s */
} lfdmi_radon_short;
void lfdmi_default_radon_short_params(lfdmi_radon_short_params *out);
/* lfdmi_radon_search with steps 10 - 12: frames, dtype, n, loc and sigma as there.  sp NULL: the defaults.  lines: n * max_lines
 * records (host), frame i's at lines[i * max_lines ..], and n_lines: n counts (host), laid out as lfdmi_radon_search_lines'
 * (step 8).  plain: NULL, or n records (host) that receive, bit for bit, what lfdmi_radon_search returns for these frames: round
 * 0 runs the last level as well.  Out-of-range parameters: LFDMI_ERR_ARG, and nothing runs.  On its first call the handle
 * allocates what lfdmi_radon_search_lines' first call does (if it has not) and the scoring levels' partial records;
 * lfdmi_radon_dims counts them from then on.  The frames are only read; the call refuses while calls are in flight, runs on
 * the context's stream and waits for it once per round of each chunk. */
int lfdmi_radon_search_short(lfdmi_ctx *ctx, lfdmi_radon *radon, const void *frames, int dtype, int n, int loc, const float *sigma,
                             const lfdmi_radon_short_params *sp, lfdmi_radon_short *lines, int32_t *n_lines,
                             lfdmi_radon_result *plain);
#define LFDMI_RADON_MAX_WIDTH 16
typedef struct {
    int32_t max_width;        /* the widest band scored, in binned cells: a power of two, 1 .. LFDMI_RADON_MAX_WIDTH; default 8 */
    int32_t max_lines;        /* records per frame at most, 1 .. LFDMI_RADON_MAX_LINES; default 4 */
    int32_t peel_halfwidth;   /* half-width in pixels blotted beyond a found band's two edges (>= 0); default 8 */
    int32_t min_seg;          /* valid pixels a segment of the band needs, 1 .. the handle's min_len; default 64 */
    float wide_threshold;     /* found = snr >= wide_threshold; finite and > 0; default 8 (step 14) */
    int32_t pad;
} lfdmi_radon_wide_params;
typedef struct {
    int32_t status;       /* as in lfdmi_radon_line, down to ey2: y0 is the band's lowest line, x1 .. theta and ex1 .. ey2 lie on */
    int32_t found;        /* its centre line (steps 15, 16), n_pix, sum and snr are the band's, found = snr >= wide_threshold */
    int32_t q, y0, s;
    int32_t n_pix;
    float sum, snr;
    double x1, y1, x2, y2, rho, theta;
    int32_t c1, c2;
    int32_t seg_n_pix;
    int32_t pad;
    float seg_sum, seg_snr;
    double ex1, ey1, ex2, ey2;
    int32_t width, pad2;  /* k: the band's width in binned cells */
    double width_px;      /* its width across the line in pixels (step 15) */
} lfdmi_radon_wide;
void lfdmi_default_radon_wide_params(lfdmi_radon_wide_params *out);
/* lfdmi_radon_search with steps 13 - 16: frames, dtype, n, loc and sigma as there.  wp NULL: the defaults.  lines, n_lines and
 * plain as in lfdmi_radon_search_short: the width-1 pass of round 0 is exactly step 5, and its best is kept beside the overall
 * one.  Out-of-range parameters: LFDMI_ERR_ARG, and nothing runs.  On its first call the handle allocates what
 * lfdmi_radon_search_lines' first call does (if it has not) and the band kernel's partial records; lfdmi_radon_dims counts them
 * from then on.  The frames are only read; the call refuses while calls are in flight, runs on the context's stream and waits
 * for it once per round of each chunk. */
int lfdmi_radon_search_wide(lfdmi_ctx *ctx, lfdmi_radon *radon, const void *frames, int dtype, int n, int loc, const float *sigma,
                            const lfdmi_radon_wide_params *wp, lfdmi_radon_wide *lines, int32_t *n_lines,
                            lfdmi_radon_result *plain);

/* null peaks: the frame's own noise ceiling.  The thresholds above rest on crops of pure Gaussian noise (steps 5, 12, 14); a
 * real frame has many more lines, what remove_stars left behind, and a sigma that is an estimate.  lfdmi_radon_null measures
 * what the very same search reaches on the frame once every line in it is destroyed: the frame is scrambled -- every pixel
 * takes the exact bits of a pixel drawn from the frame itself, so the value distribution, the share of invalid pixels and
 * sigma stay and no geometry does -- and searched, K times.  Nothing below is new arithmetic: tests/radon_null_ref.py builds
 * the scrambled frame with numpy integers and calls the restatements of the searches, and the device matches bit for bit.
 * 17. Key.  For frame f with the caller's seed[f] (uint64; without seeds, seed[f] = f) and realisation r = 0 .. K-1:
 *        k = splitmix64(seed[f] + 0x9E3779B97F4A7C15 * (r + 1)),
 *        splitmix64(x): x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *                       x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)
 *    all modulo 2^64, on the host.
 * 18. Source pixel.  N = H W (below 2^32 for every shape a handle takes).  For buffer index i = row * W + column (row: the
 *    buffer's, before step 1's flip), in uint32 arithmetic modulo 2^32 but for the last product:
 *        a = fmix32(i * 0x9E3779B1 + lo32(k));  u = fmix32(a ^ hi32(k));  j = (uint32)(((uint64)u * N) >> 32)
 *        fmix32(h): h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16     (murmur3's finaliser)
 *    j < N always.
 * 19. Scrambled frame.  X'[i] = X[j] as a 32-bit pattern (of a big-endian frame: the stored pattern, which step 1 then swaps
 *    as it does for X).  This is sampling with replacement, not a permutation: every value, valid or not, arrives with its
 *    exact bits.  X' is never stored: step 2's cells read their b x b pixels through j.
 * 20. Null record (f, r) of a kind is record 0 of that kind's search of X' with the frame's sigma[f]: LFDMI_RADON_NULL_LINES,
 *    steps 1 - 6, an lfdmi_radon_result; LFDMI_RADON_NULL_SHORT, steps 10 - 12 with max_lines = 1, an lfdmi_radon_short;
 *    LFDMI_RADON_NULL_WIDE, steps 13 - 16 with max_lines = 1, an lfdmi_radon_wide.  No peel round runs; a short or wide
 *    record with found = 1 has its segment (steps 12, 16), which at the default thresholds a null record should never be.
 *    With the null peaks snr_0 .. snr_K-1 of a frame, a line of that frame with score x has the false-alarm estimate
 *    (1 + #{snr_r >= x}) / (K + 1), which is never 0, and margin * max snr_r is the rule the default thresholds follow.
 *    Not covered: a null that keeps two-dimensional noise correlation, peel-round nulls for schemes that move pixels; no
 *    default threshold changes on these numbers.
 *
 * lfdmi_radon_null_scheme makes the null frame X' in other ways than the scramble, which keeps the frame's mean in every line
 * (a trail's or a star's leftover flux lifts the whole null), spreads the invalid pixels evenly (the frame's blots and bleed
 * columns cut particular lines short) and destroys the noise's correlation.  tests/radon_null_schemes_ref.py restates steps
 * 21 and 22.  With u(i) = fmix32(fmix32(i * 0x9E3779B1 + lo32(k)) ^ hi32(k)), step 18's u for an index i and step 17's key k:
 * 21. Schemes.  X is the buffer, r and c its row and column before step 1's flip.
 *    LFDMI_RADON_NULL_SCRAMBLE: steps 18 - 19; with n_peel = 0 the records are lfdmi_radon_null's bit for bit.
 *    LFDMI_RADON_NULL_SIGNFLIP: X'[i], i = r W + c, is X[i] with the value's sign bit inverted where u(i) >> 31 is 1 (of a
 *    big-endian frame: the sign bit of the value after step 1's swap); every other bit is kept.  Step 1's validity ignores
 *    the sign (finite, not +-0, |x| <= clip), so M of X' is M of X exactly: every line keeps its N, and every pixel its
 *    place.  What it does not do: it removes the frame's mean from the null, so a badly subtracted sky lowers the null and
 *    does not lower the search; and it does not keep the sign structure of correlated noise.
 *    LFDMI_RADON_NULL_ROWSHIFT: o(r) = (uint32)(((uint64)u(r) * W) >> 32) < W and X'[r][c] = X[r][(c + o(r)) mod W]: a
 *    permutation inside every row, which keeps the frame's values, its mean, every row's content and the correlation along
 *    rows.  What it does not do: it leaves a trail along the rows whole.
 *    LFDMI_RADON_NULL_COLSHIFT: the same along columns, o(c) = (uint32)(((uint64)u(c) * H) >> 32) < H and
 *    X'[r][c] = X[(r + o(c)) mod H][c].  What it does not do: it leaves a trail along the columns whole.  For a found line of
 *    orientation q, COLSHIFT is the scheme for q = 0, 1, whose lines cross the columns, and ROWSHIFT for q = 2, 3.
 * 22. Rounds.  Peel records are allowed only with SIGNFLIP, which keeps positions: under the other schemes the trail's pixels
 *    are no longer under its band.  peel holds n * n_peel records, frame f's at peel[f * n_peel ..], n_peel = 0 ..
 *    LFDMI_RADON_MAX_LINES.  V', M' are step 2's binning of X'.  Every record with width >= 1 has its band blotted out of V',
 *    M' exactly as step 8 does it (width = 1) or step 16 (width = k, a power of two up to LFDMI_RADON_MAX_WIDTH), with
 *    hw = ceil(peel_halfwidth / bin) of the kind's parameters; a record of width 0 is no line and is not looked at.  The
 *    kind's search of step 20 then runs on the result (a found short or wide record has its segment on it).  The null of
 *    round k of a frame is the call with that frame's lines 0 .. k-1. */
enum { LFDMI_RADON_NULL_LINES = 0, LFDMI_RADON_NULL_SHORT = 1, LFDMI_RADON_NULL_WIDE = 2 };
#define LFDMI_RADON_NULL_MAX 64
/* The null records of n frames: frames, dtype, n, loc and sigma as in lfdmi_radon_search.  seeds: n uint64 (host); NULL: frame
 * f has seed f.  K: realisations per frame, 1 .. LFDMI_RADON_NULL_MAX.  kind: LFDMI_RADON_NULL_*.  kind_params: an
 * lfdmi_radon_short_params (SHORT) or lfdmi_radon_wide_params (WIDE), checked as their searches check them (max_lines and
 * peel_halfwidth are checked and not used); NULL: the defaults; LINES takes none (it must be NULL).  records: n * K records of
 * the kind's type (host), frame f's at records[f * K ..].  Realisation r of frame f takes one of the handle's max_frames slots,
 * so n * K > max_frames runs in chunks of max_frames realisations (a frame's realisations may lie in two chunks).  The first
 * call of a kind allocates what that kind's search does; lfdmi_radon_dims counts it.  The frames are only read; the call
 * refuses (LFDMI_ERR_ARG) while calls are in flight, on a sigma that is not positive, on K or kind out of range and on
 * parameters out of range, runs on the context's stream and waits for it once, at its end. */
int lfdmi_radon_null(lfdmi_ctx *ctx, lfdmi_radon *radon, const void *frames, int dtype, int n, int loc, const float *sigma,
                     const uint64_t *seeds, int K, int kind, const void *kind_params, void *records);
enum { LFDMI_RADON_NULL_SCRAMBLE = 0, LFDMI_RADON_NULL_SIGNFLIP = 1, LFDMI_RADON_NULL_ROWSHIFT = 2, LFDMI_RADON_NULL_COLSHIFT = 3 };
typedef struct { int32_t q, y0, s, width; } lfdmi_radon_peel;   /* width 0: no line in this place */
/* lfdmi_radon_null with steps 21 and 22: everything up to kind_params as there, but that LINES takes NULL or an
 * lfdmi_radon_lines_params (checked as lfdmi_radon_search_lines checks it; its peel_halfwidth is step 22's), and the peel_halfwidth
 * of the short and wide parameters is used.  scheme: LFDMI_RADON_NULL_SCRAMBLE .. COLSHIFT.  peel: n * n_peel records (host), or
 * NULL with n_peel = 0.  LFDMI_ERR_ARG, with nothing run and nothing written: scheme out of range; n_peel outside 0 ..
 * LFDMI_RADON_MAX_LINES; n_peel > 0 with peel NULL or with a scheme other than SIGNFLIP; of a record, width not 0 or a power of
 * two up to 16, and with width >= 1, q outside 0 .. 3, s outside 0 .. P-1 or y0 outside [-(P-1), R-1] of its orientation;
 * everything lfdmi_radon_null refuses.  Slots, chunks, seeds, sigma, the allocations of the first call (with n_peel > 0 the
 * second V, M set too), the refusal while calls are in flight and the single wait at the end are lfdmi_radon_null's. */
int lfdmi_radon_null_scheme(lfdmi_ctx *ctx, lfdmi_radon *radon, const void *frames, int dtype, int n, int loc, const float *sigma,
                            const uint64_t *seeds, int K, int kind, const void *kind_params, int scheme,
                            const lfdmi_radon_peel *peel, int n_peel, void *records);

/* ---- short-streak search ----------------------------------------------------------------------------------------------------
 * The three searches above need a long trail: the detector needs pixels that survive the 8-bit conversion, lfdmi_radon_search
 * a trail that crosses the frame, and lfdmi_radon_search_short scores only strips of 64 binned columns and up that are aligned
 * to their dyadic grid (its step 10 deliberately leaves the levels of 32 columns and below alone).  lfdmi_streak_search finds
 * a streak of 20 to 120 px that starts and stops anywhere: a slow satellite in a short exposure, an asteroid trailed by the
 * drift scan, a meteor's end piece.  It sums the binned frame along every oriented segment of one length L, anchored at every
 * cell, and reports the segment of largest signal-to-noise.  The reference has no such step.  The procedure below is the
 * definition; tests/streak_ref.py restates it in numpy.  Every sum is an integer, so the device equals it in every integer and
 * in every bit of every float and double, whatever its tiling, its order of reduction or its atomics.
 *
 * 1. Pixels.  Coordinates and validity are those of faint-trail step 1: the flipped frame, a pixel valid when it is finite, not
 *    +-0 and |x| <= clip.  g = llrint((double)x * 2^20) where valid, else 0; m = 1 where valid, else 0.
 * 2. Binning by b = bin (1, 2 or 4).  Hb, Wb and the cells' pixels are those of faint-trail step 2.  G[j][i] = the integer sum
 *    of g over the cell, M[j][i] = the integer sum of m.  Range rule: llrint(clip * 2^20) * b * b * L < 2^31 (clip: the float32
 *    parameter), otherwise LFDMI_ERR_ARG; under it every sum below fits int32.  The defaults (clip 0.125, b 2, L 32) give
 *    2^24 at most.
 * 3. Orientations.  q = 0: Q[r][c] = G[r][c], R = Hb, C = Wb.  q = 1: Q[r][c] = G[c][r], R = Wb, C = Hb.  The same of M.
 * 4. Segments.  L = length, a power of two from 8 to 64.  The slope s runs over -(L-1) .. L-1, and
 *        off(i; s) = sgn(s) * ((2 |s| i + (L-1)) / (2 (L-1)))          (integer division; i = 0 .. L-1)
 *    so off(0) = 0 and off(L-1) = s.  Segment (q, s, r0, c0) is the cells Q[r0 + off(i; s)][c0 + i].  It exists only when all L
 *    cells lie inside [0, R) x [0, C): there are no partial segments, and an orientation with C < L has none.  S = the sum of Q
 *    over the segment, N = the sum of M.
 * 5. Score.  A segment is a candidate when 2 N >= L b b (the short search's half-valid rule).  A = (float)((double)S * 2^-20):
 *    one rounding.  snr = A / (sigma * sqrtf((float)N)) with faint-trail step 5's three roundings.  The frame's streak is the
 *    candidate of largest snr; ties go to the lowest (q, s + L-1, r0, c0).  Without a candidate the record is
 *    LFDMI_STREAK_NONE (snr 0, found 0, every other field 0), otherwise LFDMI_STREAK_OK.  found = snr >= threshold (float32).
 *    threshold defaults to 8: sixteen noise-only 372 x 512 frames of sigma 0.025 (the faint-trail search's figures' frames) peak,
 *    at the defaults, at 5.18 5.05 5.08 4.85 4.58 5.41 4.86 4.98 5.30 4.97 4.84 5.03 4.87 5.02 5.19 5.12; 1.4 times the largest,
 *    the margin the short search keeps, is 7.58, rounded up to the next 0.5.
 * 6. Record.  status, found, q, s, r0, c0, n_pix (N), sum (A), snr, and x1, y1, x2, y2, rho, theta (double, on the host): the
 *    working points (c0, r0) and (c0 + L-1, r0 + s) map to binned (i, j) as (c, r) for q = 0 and (r, c) for q = 1, and to pixels
 *    as b i + (b-1)/2, b j + (b-1)/2.  theta and rho follow faint-trail step 6.
 * 7. Rounds.  Up to max_streaks records per frame.  A frame goes on to round k+1 when its round-k record is LFDMI_STREAK_OK
 *    with found = 1 and k+1 < max_streaks.  With hw = ceil(peel_halfwidth / b), every cell of G and M is set to 0 whose working
 *    coordinates (r, c) in the record's orientation satisfy, with i = c - c0 and ic = min(max(i, 0), L-1),
 *        -hw <= i <= L-1+hw     and     |r - (r0 + off(ic; s))| <= hw
 *    and steps 3 - 6 run again on the peeled arrays.  n_streaks and the stopping record are laid out as
 *    lfdmi_radon_search_lines' step 8 lays out n_lines: records 0 .. n_streaks-1 have found = 1; if n_streaks < max_streaks,
 *    record n_streaks is the round that stopped the frame, and later records are all zero.  Record 0 does not depend on
 *    max_streaks.  A streak longer than L comes back as consecutive pieces; joining them is left to the caller. */
enum { LFDMI_STREAK_OK = 0, LFDMI_STREAK_NONE = 1 };
#define LFDMI_STREAK_MAX_STREAKS 8
typedef struct {
    int32_t bin;              /* 1, 2 or 4; default 2: binning is the search's width knob */
    int32_t length;           /* L in binned cells: 8, 16, 32 or 64; default 32 */
    int32_t max_streaks;      /* records per frame at most, 1 .. LFDMI_STREAK_MAX_STREAKS; default 4 */
    int32_t peel_halfwidth;   /* half-width in pixels of the footprint blotted around a found streak, 0 .. 65536; default 8 */
    float clip;               /* pixels above it in magnitude are not summed (> 0, step 2's range rule); default 0.125 */
    float threshold;          /* found = snr >= threshold; finite and > 0; default 8 (step 5) */
} lfdmi_streak_params;
typedef struct {
    int32_t status;       /* LFDMI_STREAK_* */
    int32_t found;
    int32_t q, s, r0, c0; /* the segment in working coordinates (steps 3, 4) */
    int32_t n_pix;        /* N: valid pixels on it */
    float sum, snr;       /* A and its score */
    int32_t pad;
    double x1, y1, x2, y2, rho, theta;
} lfdmi_streak;
void lfdmi_default_streak_params(lfdmi_streak_params *out);
/* frames: n frames of h x w, LFDMI_F32 or LFDMI_F32_BE, loc LFDMI_HOST / LFDMI_HOST_PINNED / LFDMI_DEVICE; only read.  sigma: n
 * float32 (host), > 0; NULL: 0.025 for every frame.  p NULL: the defaults.  out: n * max_streaks records (host), frame i's at
 * out[i * max_streaks ..]; n_streaks: n counts (host).  LFDMI_ERR_ARG, and nothing runs: parameters out of range (the range
 * rule among them), a sigma that is not positive, h or w below 2 bin or above 4096 bin (r0 and c0 take 12 bits each of the key
 * that orders the candidates).  The call keeps no state (its device memory comes from the stream's pool and goes back before
 * it returns), splits into chunks of frames by the unit limits (staging of host frames, bytes of binned cells), refuses
 * while calls are in flight, runs on the context's stream and waits for it once per round of each chunk (the host decides
 * which frames continue). */
int lfdmi_streak_search(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const float *sigma,
                        const lfdmi_streak_params *p, lfdmi_streak *out, int32_t *n_streaks);
/* the anchors a workgroup of the search kernel owns (rows x columns of the working array); any pointer may be NULL */
void lfdmi_streak_tile(int32_t *rows, int32_t *cols);

/* ---- stacked cross-sections -------------------------------------------------------------------------------------------------
 * lfdmi_measure_trails needs every 64-position piece of a trail to stand 5 sigma on its own; a trail of the faint-trail search
 * never does.  lfdmi_stack_profiles measures such a trail's cross-section by the Radon idea turned by 90 degrees: the frame is
 * summed ALONG a given segment, separately for every perpendicular offset, so the per-pixel noise averages down by the square
 * root of the length in every bin.  It is a measurement for trails below `clip` per pixel (brighter pixels are not summed).
 * The reference has no such step.  The procedure below is the definition; tests/stack_ref.py restates it in numpy and the
 * device matches it bit for bit.  Notation: P = prof_half, K = P / step (an integer), nb = 2K+1 bins.
 *
 * 1. Pixels.  Coordinates are the detection records': x = column, y = row of the flipped frame, so (x, y) is buffer row H-1-y.
 *    A pixel is valid when it is finite, not +-0 and |v| <= clip (float32; clip = +inf: no clipping): step 1 of the faint-trail
 *    search.
 * 2. Geometry, on the host in double, each operation rounded, no contraction.  A segment whose end points are not finite,
 *    exceed 1e6 in magnitude or coincide: LFDMI_STACK_BAD_SEGMENT.  The major axis is x when |x2-x1| >= |y2-y1|, else y; a is
 *    the coordinate along it, b the other one, A and B the frame's sizes along them; (a1, b1), (a2, b2) the end points as given.
 *    g = (b2-b1) / (a2-a1), cosphi = 1 / sqrt(1 + g*g), inv = 1 / step.  The columns are the integers a in [a_first, a_last],
 *    a_first = max(ceil(min(a1, a2)), 0), a_last = min(floor(max(a1, a2)), A-1); n_col of them; n_col < min_cols:
 *    LFDMI_STACK_TOO_SHORT.  The centre of column a is bc(a) = b1 + g*((double)a - a1).
 * 3. Bins.  u_k = (k - K) * step, k = 0 .. 2K.  A valid pixel (a, b), 0 <= b < B, falls in bin k = floor(t),
 *    t = ((double)b - bc(a)) * cosphi * inv + (K + 0.5) (left to right), when 0 <= t < 2K+1; otherwise in none.
 * 4. Sums.  The columns split into a left half [a_first, amid-1] and a right half [amid, a_last], amid = (a_first + a_last + 1)
 *    >> 1.  Within a half the columns group into blocks by a >> 5.  Per (half, block, bin): one sequential float32 accumulator
 *    from +0 over the bin's valid pixels, columns ascending, b ascending within a column.  Per (half, bin): the block sums are
 *    added in ascending block order into one sequential float32 accumulator from +0.  Counts are exact int32.  A pass yields
 *    A_L, A_R, N_L, N_R, each [2K+1].
 * 5. Refinement, on the host in double; passes i = 0 .. n_iter, the last one only measures.  In pass i < n_iter, per half:
 *    m_k = (double)A_k / (double)N_k where N_k > 0; bkg = the lower median (rank floor((m-1)/2), as in lfdmi_measure_trails) of
 *    m_k over the wing bins |u_k| >= P - wing with N_k > 0.  With hb = floor(box / (2 step)) the box score of bin k is
 *    (SA - bkg * SN) / sqrt(SN), SA / SN = the sums of (double)A_j / (double)N_j over j = max(k-hb, 0) .. min(k+hb, 2K)
 *    ascending; the half's centre is the bin k of largest score among those with |u_k| <= max_shift and SN > 0, ties to the
 *    lowest k; its shift is u_k.  Refinement stops -- this pass's sums are the result, the line stays -- when a half has no
 *    wing bin or no scored bin, when either score is below k_ref * (double)sigma, or when the new line has |g| > 2.  Otherwise,
 *    with the halves' middle columns aL = (a_first + (amid-1)) * 0.5, aR = (amid + a_last) * 0.5 and bL = bc(aL) + uL / cosphi,
 *    bR = bc(aR) + uR / cosphi: a1 = aL, b1 = bL, g = (bR - bL) / (aR - aL), cosphi from g as in step 2.  The major axis and
 *    the column range are kept.
 * 6. Result, from the last pass run.  A_k = A_L + A_R (one float32 addition), N_k = N_L + N_R, m_k = A_k / (float)N_k
 *    (float32), NaN when N_k = 0.  background (lower median of the non-NaN m_k over the wing bins), v_k = m_k - background
 *    (float32; the profile row), peak, noise (1.4826 * lower median of |v_k| over the same wing bins), fwhm (the calc_fwhm
 *    rule), fwhm_arcsec and depth exactly as step 5 of the trail profiles defines them.  status LFDMI_STACK_TOO_FAINT unless
 *    peak > 0 and peak >= k_sig * noise; such a record keeps every measured value (it is a verdict, not a failure).  flux =
 *    step * the sum of (double)v_k over the core bins |u_k| < P - wing, k ascending (the trail's flux per pixel of length);
 *    flux_err = step * noise * sqrt(number of core bins); snr = flux / flux_err.  (x1, y1), (x2, y2): the final line's points
 *    at a_first and a_last; d = their difference over its length (sqrt of the sum of squares), n = (d.y, -d.x) turned so that
 *    n.y > 0 or (n.y == 0 and n.x > 0), theta = atan2(n.y, n.x), rho = x1 n.x + y1 n.y.  With am = (a_first + a_last) * 0.5
 *    and index 0 the line as given: shift = (bc(am) - bc_0(am)) * cosphi_0 px, tilt = atan(g) - atan(g_0) rad.  min_valid = the
 *    least N_k.  Records with LFDMI_STACK_BAD_SEGMENT or _TOO_SHORT have every double NaN, a NaN row, zero sums and counts.
 *
 * The device sums 32 columns by the band's cross extent per workgroup through LDS (k_stack_block), a pixel reaching exactly one
 * bin: no float atomics, and step 4's order is kept; k_stack_combine adds the block sums. */
#define LFDMI_STACK_MAX_HALF 40.0   /* prof_half + step / 2 at most (the band of 32 columns is kept in LDS) */
enum { LFDMI_STACK_OK = 0, LFDMI_STACK_BAD_SEGMENT = 1, LFDMI_STACK_TOO_SHORT = 2, LFDMI_STACK_TOO_FAINT = 3 };
typedef struct {
    int32_t frame;            /* 0 .. n-1 */
    int32_t pad;
    double x1, y1, x2, y2;    /* flipped frame, as lfdmi_radon_line.ex1 .. ey2, a results row or an injected trail's truth */
} lfdmi_stack_segment;
typedef struct {
    int32_t wing;             /* wing width in px for background and noise (1 .. < prof_half); default 8 */
    int32_t n_iter;           /* refinement passes (0 .. 16); default 2 */
    int32_t min_cols;         /* columns a segment needs (>= 2); default 64 */
    float clip;               /* pixels above it in magnitude are not summed (> 0, +inf allowed); default 0.125 */
    double prof_half;         /* P: profile half-width in px; default 24 */
    double step;              /* bin step in px (> 0; P / step an integer, 1 .. 512; P + step / 2 <= LFDMI_STACK_MAX_HALF); default 0.5 */
    double box;               /* window of the refinement's box score in px (>= 0); default 4 */
    double max_shift;         /* the refinement looks within |u| <= max_shift px (>= 0); default 8 */
    double k_sig;             /* TOO_FAINT below peak = k_sig * noise; default 6.  The restatement on 372 x 512 frames of sigma 0.025,
                                 start line off by 1.5 px and 0.15 degrees: 16 noise-only frames peak / noise 1.7 - 3.7, 16 trails of
                                 peak 0.02 (Gaussian sigma 2 px) 9.2 - 18.4 */
    double k_ref;             /* a half moves the line when its box score reaches k_ref * sigma; default 4.  The same frames: the
                                 smaller half score over sigma 0.1 - 2.0 (noise), 17.2 - 23.4 (trails) */
    double pixscale;          /* arcsec per px; default 0.396 (SDSS) */
} lfdmi_stack_params;
typedef struct {
    int32_t status;           /* LFDMI_STACK_* */
    int32_t n_col;            /* columns summed */
    int32_t min_valid;        /* fewest pixels in any bin */
    int32_t n_pass;           /* passes run (1 .. n_iter + 1) */
    double rho, theta;        /* the refined line */
    double x1, y1, x2, y2;    /* its points at the first and last column */
    double background, noise, peak;
    double fwhm, fwhm_arcsec, depth;
    double flux, flux_err, snr;
    double shift, tilt;       /* how far the refinement moved the line: px at the middle column, rad */
} lfdmi_stack;
void lfdmi_default_stack_params(lfdmi_stack_params *out);
/* frames: n frames of h x w, LFDMI_F32 or LFDMI_F32_BE, loc LFDMI_HOST / LFDMI_HOST_PINNED / LFDMI_DEVICE; only read.  segs: n_seg
 * segments (host), any number per frame.  sigma: n float32 (host), the sky sigma of each frame, > 0; NULL: 0.025.  p NULL: the
 * defaults.  out: n_seg records (host).  profiles: n_seg x (2K+1) float32, the rows v_k; sums / counts: n_seg x 2 x (2K+1)
 * float32 / int32, A_L, A_R / N_L, N_R of the last pass (host; each may be NULL).  Out-of-range parameters, a segment's frame
 * outside [0, n), a sigma that is not positive: LFDMI_ERR_ARG, and nothing runs.  The call keeps no state (its device memory
 * comes from the stream's pool and goes back before it returns), refuses while calls are in flight, runs on the context's
 * stream and waits for it once per pass (the host refines the lines in between). */
int lfdmi_stack_profiles(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_stack_segment *segs,
                         int n_seg, const float *sigma, const lfdmi_stack_params *p, lfdmi_stack *out, float *profiles, float *sums,
                         int32_t *counts);

/* ---- source finder ------------------------------------------------------------------------------------------------------------
 * remove_stars blots the sources a photoObj table lists; a frame that has no such table (a raw exposure, an fpC file, another
 * survey's frame) gets its catalogue from here: the compact sources of the frame itself, as an lfdmi_catalog the existing
 * remove_stars path takes unchanged.  The reference has no such step.  The procedure below is the definition;
 * tests/stars_ref.py restates it in numpy and the device matches it bit for bit: every float32 sum has a fixed order, every
 * other statistic is a comparison or a maximum.
 *
 * Input: frame x of H x W float32 in buffer rows (not flipped: what remove_stars sees), pixel (y, c) = x[y][c].  sigma: the sky
 * sigma of the frame (NULL: 0.025f for every frame).  A non-finite pixel and a pixel outside the frame count as +0 in every step.
 * (Frames whose 3 x 3 sums overflow float32 are outside the definition.)
 *
 * 1. Smoothing.  h[y][c] = (x[y][c-1] + x[y][c]) + x[y][c+1] and S[y][c] = (h[y-1][c] + h[y][c]) + h[y+1][c], float32, every
 *    addition rounded.
 * 2. Candidates.  T = (float)(k_det * 3.0 * (double)sigma): k_det sigmas of S on a flat sky, whose 9 pixels add to 3 sigma.
 *    Pixel p is a candidate when, over the window |dy| <= sep, |dx| <= sep clipped to the frame, S[p] >= T, S[p] > S[q] for every
 *    window pixel q before p in raster order and S[p] >= S[q] for every window pixel q after p: a tie goes to the first pixel in
 *    raster order, and a flat plateau yields only its leading pixels.
 * 3. Order and cap.  A frame's candidates are numbered in raster order (y, then c); the first max_obj are reported.  The frame
 *    record carries n_found (all candidates), n_out = min(n_found, max_obj) and the status LFDMI_STARS_OK or
 *    LFDMI_STARS_TRUNCATED (n_found > max_obj).
 * 4. Radius.  E = max((float)(edge_frac * (double)S[p]), (float)(k_edge * 3.0 * (double)sigma)).  For r = 1 .. r_max, M_r = the
 *    maximum of S over the frame's pixels at Chebyshev distance r from p (-inf when there is none).  rad = the smallest r with
 *    M_r < E; if there is none the candidate is LFDMI_STAR_EXTENDED and rad = 0 (a trail crosses every ring, so its ridge maxima
 *    end here, and so do bleed columns and galaxies larger than r_max).  LFDMI_STAR_EDGE: the square |d| <= rad is clipped by the
 *    frame.
 * 5. Measurement over the square |dy|, |dx| <= rad clipped to the frame (an extended candidate: the peak pixel alone), v = the
 *    pixel.  Per row, float32, dx ascending from +0: a_y = sum v, b_y = sum (v * (float)dx), each product rounded and then added
 *    (no FMA).  Then in double, dy ascending from 0: F = sum a_y, MX = sum b_y, MY = sum (double)dy * (double)a_y.  flux =
 *    (float)F; if F > 0, xc = (float)(px + MX / F) and yc = (float)(py + MY / F), otherwise the peak's x and y.
 * 6. Record.  lfdmi_star below; s_peak = S[p].
 * 7. Parameters.  lfdmi_stars_params below.
 * 8. Catalogue (lfdmi_stars_catalog).  max_obj rows per frame, count = n_out.  A row without LFDMI_STAR_EXTENDED: nobserve =
 *    ndetect = 1; the five psfmag 0 (under every filter cap, every pair difference 0); the five petro90 = (float)((double)rad *
 *    pixscale); the five colc = (float)y and the five rowc = (float)x -- remove_stars takes ceil(COLC) on axis 0, so the row goes
 *    into colc.  With the default params_removestars the blotted square then has half-width int(ceil(rad * 0.396) / 0.396) + 10:
 *    at least rad + 10 and at most 42, under maxxy = 60 for rad <= 32.  A row with LFDMI_STAR_EXTENDED: nobserve = 0, ndetect = 1,
 *    so it is never blotted.  Rows past count are zero, but for ndetect = 1.  remove_stars slices img[x-d : x+d] as Python does:
 *    a start below zero counts from the far edge and the slice is empty, so a source closer than its half-width d (rad + 10 or
 *    more) to the top or the left edge of the buffer is not blotted -- with this catalogue as with a photoObj one.
 *
 * The device reads a frame once per 64 x 16 tile with a halo of sep + 1 (k_stars_detect: 4 H W bytes per frame is the floor), keeps
 * one bit per pixel, ranks the bits by a scan over the rows (k_stars_rows) and measures one source per workgroup from a
 * (2 r_max + 3)^2 patch in LDS (k_stars_measure); k_stars_catalog is step 8.  No kernel uses an atomic or a transcendental. */
#define LFDMI_STARS_MAX_OBJ 1048576
enum { LFDMI_STARS_OK = 0, LFDMI_STARS_TRUNCATED = 1 };
enum { LFDMI_STAR_EXTENDED = 1, LFDMI_STAR_EDGE = 2 };
typedef struct {
    double k_det;             /* detection threshold in sigmas of S (> 0); default 5 */
    double k_edge;            /* a source ends where its rings fall below k_edge sigmas of S (> 0); default 3 */
    double edge_frac;         /* ... or below this share of its peak, whichever is higher (0 .. 1); default 0.02 */
    int32_t sep;              /* half-width of the local-maximum window (1 .. 8); default 3 */
    int32_t r_max;            /* largest radius (1 .. 32); default 32 */
    int32_t max_obj;          /* records per frame (1 .. LFDMI_STARS_MAX_OBJ); default 4096 */
} lfdmi_stars_params;
typedef struct {
    int32_t x, y;             /* the peak: column and row of the buffer */
    int32_t rad;              /* 1 .. r_max, 0 for an extended candidate */
    int32_t flags;            /* LFDMI_STAR_* */
    float s_peak, flux, xc, yc;
} lfdmi_star;
typedef struct {
    int32_t status;           /* LFDMI_STARS_* */
    int32_t n_found, n_out;
} lfdmi_stars_frame;
void lfdmi_default_stars_params(lfdmi_stars_params *out);
/* frames: n frames of h x w, LFDMI_F32 or LFDMI_F32_BE, loc LFDMI_HOST / LFDMI_HOST_PINNED / LFDMI_DEVICE; only read.  sigma: n
 * float32 (host), > 0; NULL: 0.025.  p NULL: the defaults.  out_records: n x max_obj records at out_loc (host or device), rows past
 * n_out zero; frame_records: n records (host).  Out-of-range parameters, a sigma that is not positive: LFDMI_ERR_ARG, and nothing
 * runs.  The call keeps no state (its device memory comes from the stream's pool and goes back before it returns), refuses while
 * calls are in flight, runs on the context's stream and waits for it twice per chunk of frames. */
int lfdmi_find_stars(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const float *sigma,
                     const lfdmi_stars_params *p, lfdmi_star *out_records, int out_loc, lfdmi_stars_frame *frame_records);
/* step 8: fills the arrays cat points at ([n][max_obj][5] / [n][max_obj] / count [n], in host or device memory as cat->loc says;
 * cat->max_obj == max_obj) from n x max_obj records at rec_loc and the n frame records (host).  n at most 32768. */
int lfdmi_stars_catalog(lfdmi_ctx *ctx, const lfdmi_star *records, int rec_loc, const lfdmi_stars_frame *frame_records, int n,
                        int max_obj, double pixscale, const lfdmi_catalog *cat);

/* ---- frame seeing -------------------------------------------------------------------------------------------------------------
 * The defocus fit takes a per-trail seeing (lfdmi_fit_defocus: NaN leaves it free), and one cross-section cannot tell seeing
 * from defocus: both widen it alike.  The frame's stars can: each is an image of the seeing disc.  lfdmi_measure_seeing
 * measures the second moments of the frame's good stars, as the source finder's records name them, before remove_stars blots
 * them.  The reference has no such step.  The procedure below is the definition; tests/psf_ref.py restates it in numpy.
 * Everything that leaves the device is an integer, so the device matches the restatement in every bit; the few doubles of the
 * host step (5) have a fixed order.
 *
 * Input: the frames lfdmi_find_stars saw (buffer rows, not flipped), per frame max_obj records of lfdmi_star and the frame's
 * lfdmi_stars_frame record (its n_out, 0 .. max_obj, is the number of records read), and the sky sigma of the finder.
 *
 * 1. Pixels.  A pixel v enters as q = llrint((double)v * 2^30), as in the light curves (step 1 there).  A pixel is bad when it is
 *    not finite, is +-0 (what remove_stars or a mask fill blotted) or has |v| > sat.  sat <= 4096, so |q| <= 2^42 and |q - b|
 *    <= 2^43; with dx^2, dy^2 <= 2^8 and at most 33^2 < 2^11 pixels in a window, every int64 sum below stays under 2^43 * 2^8 *
 *    2^11 = 2^62 < 2^63 (the ring's sum: at most 65^2 < 2^13 pixels, under 2^55).
 * 2. Status of record i of a frame, the first rule that applies; H = win + gap + ring:
 *      LFDMI_PSF_NOT_CANDIDATE  flags != 0, rad == 0, rad > rad_max, or not s_peak >= (float)(k_peak * 3.0 * (double)sigma)
 *      LFDMI_PSF_CLIPPED        the square |dx|, |dy| <= H around the peak (x, y) leaves the frame
 *      LFDMI_PSF_CROWDED        another record j < n_out of the frame (whatever its flags) has max(|x_j - x|, |y_j - y|) <= iso
 *      LFDMI_PSF_BAD_PIXEL      a pixel of the square is bad
 *      LFDMI_PSF_OK             otherwise
 * 3. Sums of an OK record, d = max(|dx|, |dy|) the Chebyshev distance from the peak.  Ring, win + gap < d <= H: n_ring pixels,
 *    Q_ring = sum q, b = Q_ring / n_ring as C divides (towards zero).  Window, d <= win, p = q - b: Q0 = sum p, Qx = sum p dx,
 *    Qy = sum p dy, Qxx = sum p dx^2, Qyy = sum p dy^2, Qxy = sum p dx dy.  All int64: no order matters.
 * 4. Frame.  The first max_used OK records in record order are packed into the output (lfdmi_psf_star, index = i; rows past
 *    n_packed are zero).  n_ok counts the OK records, n_cand those that are not NOT_CANDIDATE, and every status is counted.
 * 5. Host, in double, every operation rounded (no FMA), for the packed stars in their order:
 *      mx = Qx / Q0, my = Qy / Q0 (each sum converted to double first); sxx = Qxx / Q0 - mx * mx, syy = Qyy / Q0 - my * my,
 *      sxy = Qxy / Q0 - mx * my; t = sxx + syy, d = sxx - syy, e = sqrt(d * d + 4.0 * (sxy * sxy)) / t.
 *    A star is used when Q0 > 0, sxx > 0, syy > 0 and e <= e_max; its width is 2.3548200450309493 * sqrt(t / 2.0)
 *    (2 sqrt(2 ln 2) times the mean sigma).  fwhm_px = the lower median of the used widths (sorted ascending, element
 *    (n_used - 1) / 2); scatter = 1.4826 times the lower median of |width - fwhm_px|; ell = the lower median of e.  All three
 *    are NaN when n_used = 0.  status = LFDMI_SEEING_FEW when n_used < min_stars (fwhm_px is reported all the same; whoever
 *    hands a seeing to the fit leaves it free then), otherwise LFDMI_SEEING_OK.
 *    The window truncates a star's wings and the pixel widens it, so fwhm_px is not the seeing FWHM the defocus bank is
 *    built on: lfd_amd/psf.py (to_bank_seeing) applies this very measurement to noise-free renderings of the bank's S and
 *    inverts the table.
 *
 * The device runs one wavefront per record (k_psf_measure: the rules of step 2 in order, the crowding test with a lane per
 * other record, the square row by row with the byte swap on load, seven int64 sums added across the wave by shuffles) and one
 * workgroup per frame for step 4 (k_psf_pack: ballot and prefix count).  No kernel uses an atomic, a transcendental or float
 * arithmetic beyond the comparison of s_peak.  What bounds either kernel has not been measured. */
enum { LFDMI_PSF_OK = 0, LFDMI_PSF_NOT_CANDIDATE = 1, LFDMI_PSF_CLIPPED = 2, LFDMI_PSF_CROWDED = 3, LFDMI_PSF_BAD_PIXEL = 4 };
enum { LFDMI_SEEING_OK = 0, LFDMI_SEEING_FEW = 1 };
#define LFDMI_PSF_MAX_SAT 4096.0
typedef struct {
    double k_peak;            /* a candidate's s_peak in sigmas of S (> 0); default 50 */
    double e_max;             /* largest ellipticity of a used star (0 .. 1); default 0.2 */
    double sat;               /* a pixel with |v| above it is bad (> 0, at most LFDMI_PSF_MAX_SAT = the default: off) */
    int32_t win;              /* half-width of the moment window (1 .. 16); default 7 */
    int32_t gap;              /* pixels between window and ring (0 .. 8); default 2 */
    int32_t ring;             /* width of the background ring (1 .. 8); default 3 */
    int32_t iso;              /* no other record within this Chebyshev distance (1 .. 64); default 12 */
    int32_t rad_max;          /* largest finder radius of a candidate (1 .. 32); default 16 */
    int32_t min_stars;        /* fewer used stars: LFDMI_SEEING_FEW (1 .. 1024); default 5 */
    int32_t max_used;         /* packed stars per frame (1 .. 1024); default 256 */
    int32_t pad;
} lfdmi_psf_params;
typedef struct {
    int32_t index;            /* the record's index in its frame */
    int32_t n_ring;
    int64_t Q0, Qx, Qy, Qxx, Qyy, Qxy, Q_ring;
} lfdmi_psf_star;
typedef struct {
    int32_t status;           /* LFDMI_SEEING_* */
    int32_t n_cand, n_ok, n_packed, n_used;
    int32_t n_not_candidate, n_clipped, n_crowded, n_bad_pixel;   /* with n_ok: the frame's n_out records by status */
    int32_t pad;
    double fwhm_px, scatter, ell;
} lfdmi_seeing_frame;
void lfdmi_default_psf_params(lfdmi_psf_params *out);
/* frames, dtype, loc, sigma: as lfdmi_find_stars takes them; only read.  records: n x max_obj lfdmi_star at rec_loc (host or
 * device: the finder's out_loc, so the chain stays on the device); frame_records: the finder's n records, always on the host,
 * where lfdmi_find_stars writes them and lfdmi_stars_catalog reads them (rec_loc says nothing about them).  p NULL: the
 * defaults.  out_stars: n x max_used records (host); out_frames: n records (host).  Out-of-range parameters, a sigma that is not
 * positive, an n_out outside [0, max_obj]: LFDMI_ERR_ARG, and nothing runs.  The call keeps no state (its device memory comes
 * from the stream's pool and goes back before it returns), refuses while calls are in flight, runs on the context's stream and
 * waits for it once per chunk of frames.  Chunks: host frames by stage_bytes (1 GiB), host records and the per-record sums by
 * stars_rec_bytes (256 MiB: max(1, bytes / (max_obj * 64)) frames); lfdmi_debug_unit_split's out[0] counts them. */
int lfdmi_measure_seeing(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const float *sigma,
                         const lfdmi_star *records, int rec_loc, const lfdmi_stars_frame *frame_records, int max_obj,
                         const lfdmi_psf_params *p, lfdmi_psf_star *out_stars, lfdmi_seeing_frame *out_frames);

/* ---- detection rounds -------------------------------------------------------------------------------------------------------
 * lfdmi_detect_batch* reports at most one trail per frame: process_field_bright / _dim stop at the first line set that passes,
 * as the reference does.  lfdmi_detect_rounds reports up to max_trails: it detects, blots the band of every line found so far
 * on a work copy of the frame, and detects again, until a round finds nothing.  It is built from pieces that exist: a round is
 * the plain lfdmi_detect_batch_raw; a band is the trail masks' band (steps 2 and 3 there); a pixel set to +0 is blotted for the
 * detector exactly as a remove_stars square is.  The reference has no such step.  The procedure below is the definition;
 * tests/rounds_ref.py restates it with the oracle's detector and tests/mask_ref.py's membership, and the device reproduces it
 * field for field.
 *
 * params = {max_trails 1 .. LFDMI_ROUNDS_MAX_TRAILS (default 4); half, finite and >= 0 (default 10.0: masks.half_width without a
 * measurement); dup_dist, finite and >= 0 (default 20.0)}; NULL: the defaults.  Outputs, all on the host: records
 * [n][max_trails] lfdmi_result, n_found [n] int32, dup_of [n][max_trails] int32.
 *
 * 1. Round 0 is lfdmi_detect_batch_raw(ctx, frames, dtype, n, h, w, cat, rs, bright, dim, ., loc), unchanged: records[i][0] is
 *    its record, byte for byte, and the caller's frames end the whole call in exactly the state that plain call leaves them in
 *    (blotted, swapped in place or untouched, by dtype and loc).  No band is ever written into the caller's frames.
 * 2. A record counts as found when status == 0 && found != 0.  Frame i continues into round k >= 1 when its records 0 .. k-1
 *    are all found and k < max_trails.  n_found[i] = the number of leading found records.  The record at n_found[i], if there
 *    is one, is the round that found nothing (or failed), kept as returned; the records after it are zero-filled.
 * 3. records[i][k] of a frame that continues is exactly what lfdmi_detect_batch_raw returns for the modified frame i and the
 *    same catalogue entry.  The modified frame is frame i as native float32 with every pixel inside the band of any line
 *    0 .. k-1 set to +0.0f.  Band j has the trail masks' geometry and membership (steps 2 and 3 of that section) for the
 *    segment (x1, y1) - (x2, y2) of record j converted to double (flipped-frame coordinates), with this call's half and
 *    cap = +inf: the whole line.  A record whose segment the masks would call bad (L == 0, a coordinate beyond 1e6) has no band.
 * 4. dup_of[i][k], for a found record k >= 1: the smallest j < k such that both end points (x1, y1) and (x2, y2) of record k
 *    satisfy |u| <= dup_dist, u the trail masks' step-3 expression against record j's segment, evaluated on the host in double;
 *    -1 when there is none, for k = 0 and for every record that is not found.  The end points of a record lie about 1000 px off
 *    the image along the line, so the test means "nearly the same line, within a fraction of a degree": what the wings of a
 *    trail give once the band is narrower than the trail.  dup_of is a label only; it changes no control flow.
 * 5. max_trails == 1 is the plain call and allocates nothing.  Refused before any work, the call named in the message and no
 *    output written: with LFDMI_ERR_ARG a bad params field, NULL outputs, a dtype other than LFDMI_F32 / LFDMI_F32_BE, calls in
 *    flight; with its own code everything lfdmi_detect_batch_raw refuses (its message follows "lfdmi_detect_rounds: ").
 *
 * Every round k >= 1 gathers from the caller's frames with all bands 0 .. k-1 (k_rounds_gather): the m frames that continue go
 * to work slots 0 .. m-1 in frame order, byte-swapped when the source is big-endian, +0 where a band holds the pixel centre, in
 * one pass of 4 B read and 4 B written per pixel.  No slot is compacted onto another.  Host and pinned frames: only the frames
 * that continue are uploaded, straight into their slots, and the kernel runs in place.  The band geometry (x1, y1, e, nrm, half,
 * at most 7 per slot) comes from the host as doubles; the device evaluates no division and no transcendental function.  A
 * workgroup owns a 256 x 16 tile, tests it conservatively against each band as k_mask_cull does, copies a tile no band reaches
 * with 16 B accesses and evaluates the membership per pixel, in double, left to right, uncontracted, in the others.  Rows that
 * start off a 16 B boundary (h * w % 4 != 0) get their head and tail with 4 B accesses.  The round then calls
 * lfdmi_detect_batch_raw(ctx, work, LFDMI_F32, m, h, w, cat_m, rs, bright, dim, ., LFDMI_DEVICE) with the catalogue compacted to
 * the m frames where it lives (a host gather or device copies); blotting a blotted pixel again changes nothing, so this one
 * route serves every dtype and loc.  The work buffer and the compacted device arrays come from the stream's pool, sized by m,
 * and go back after the round.  Later rounds cost what the frames still alive cost.  The call refuses while calls are in
 * flight and is synchronous; there is no non-blocking twin and no multi-scale form. */
#define LFDMI_ROUNDS_MAX_TRAILS 8
typedef struct {
    int32_t max_trails;       /* 1 .. LFDMI_ROUNDS_MAX_TRAILS; default 4 */
    int32_t pad;
    double half;              /* half-width of a found line's band in px (finite, >= 0); default 10.0 */
    double dup_dist;          /* step 4 (finite, >= 0); default 20.0 */
} lfdmi_rounds_params;
void lfdmi_default_rounds_params(lfdmi_rounds_params *out);
int lfdmi_detect_rounds(lfdmi_ctx *ctx, void *frames, int dtype, int n, int h, int w, const lfdmi_catalog *cat,
                        const lfdmi_rs_params *rs, const lfdmi_params *bright, const lfdmi_params *dim,
                        const lfdmi_rounds_params *params, lfdmi_result *records, int32_t *n_found, int32_t *dup_of, int loc);

/* ---- frame previews ---------------------------------------------------------------------------------------------------------
 * A detection ends as a row of numbers; whoever has to judge it needs to see the frame.  lfdmi_frame_previews turns frames into
 * small 8-bit images -- binned, with robust limits, through a stretch table -- while they are on the device, so that a chunk that
 * was decompressed there never has to come back at full size.  The reference leaves this to its user (its image checker browses
 * PNG files somebody else made).  Overlays and PNG files are made on the host from these images (lfd_amd/previews.py).  The
 * procedure below is the definition; tests/preview_ref.py restates it in numpy and the device reproduces every byte and every
 * integer: a pixel enters as a fixed-point integer, the cell sums are integer sums, the limits are an exact selection, and the
 * one division and one multiplication of step 5 are IEEE doubles.  No transcendental function appears: any stretch is the
 * caller's table.
 *
 * params = {bin b, one of 1, 2, 4, 8, 16 (default 4); mode LFDMI_PREVIEW_RANK (default) or LFDMI_PREVIEW_GIVEN; lo_ppm, hi_ppm,
 * 0 <= lo_ppm <= hi_ppm <= 1000000 (defaults 10000 and 995000, the percentiles strips.to_uint8 uses; read in RANK mode, checked
 * in both)}; NULL: the defaults.
 *
 * 1. Geometry.  The preview shows the flipped frame, the coordinates of every record and of results.txt: flipped row y is buffer
 *    row H-1-y.  Hp = ceil(H / b), Wp = ceil(W / b).  Preview row r, column i is the cell of the flipped rows [r b, min((r+1) b,
 *    H)) and the columns [i b, min((i+1) b, W)): the last row and column of cells may be partial.
 * 2. Pixels.  A pixel v is valid when it is finite (a big-endian frame: after the byte swap).  A blotted +0 is valid: the preview
 *    shows what the detector saw.  A valid pixel enters as the integer
 *        q = llrint(min(max((double)v, -16777216.0), 16777216.0) * 1073741824.0)      (clamped to +-2^24, times 2^30, ties to even),
 *    the light curves' and strips' convention with a clamp, so |q| <= 2^54 and the 256 pixels of the largest cell stay inside
 *    int64 (|sum| <= 2^62).  +-inf and NaN are not valid; a finite value beyond the clamp enters as +-2^54.
 * 3. Cells.  Q = the sum of q over the cell's valid pixels, c = their count.  c == 0: the cell is EMPTY, its byte is 0, its value
 *    in the cell plane is INT64_MIN, and it takes no part in step 4.  Otherwise m = Q / c as C divides int64 (towards zero).
 *    |m| <= 2^54, so INT64_MIN is no cell's mean.
 * 4. Limits of a frame.  M = the number of cells that are not EMPTY.  M == 0: the frame is LFDMI_PREVIEW_EMPTY (every byte 0).
 *    RANK: over the M values m in ascending order (rank 0 the smallest), lo = rank (lo_ppm * (M-1)) / 1000000 and hi = rank
 *    (hi_ppm * (M-1)) / 1000000, the products and quotients in int64.  A selection: equal values are equal, so no result depends
 *    on an order.  An EMPTY frame has lo = hi = 0.
 *    GIVEN: limits[2 i], limits[2 i + 1] are frame i's lo and hi as doubles x, each entering as llrint(min(max(x, -16777216.0),
 *    16777216.0) * 1073741824.0); an EMPTY frame keeps them.  One stretch across a run, such as -2 sigma .. +10 sigma.
 *    hi <= lo (and M > 0): the frame is LFDMI_PREVIEW_FLAT and every byte is 0.  Otherwise LFDMI_PREVIEW_OK.
 * 5. Level of a cell that is not EMPTY in an OK frame:
 *        d = min(max(m, lo), hi) - lo;   r = hi - lo;   k = (int)(((double)d / (double)r) * 4095.0)
 *    (int64 differences, at most 2^55; each converted to double with one rounding; one division, one multiplication, both
 *    rounded, no contraction; the cast truncates).  0 <= k <= 4095 and the byte is lut[k].
 * 6. Record of a frame: status, n_cells = M, n_empty = Hp Wp - M, lo and hi as the int64 of step 4, and lo_f = (double)lo *
 *    2^-30, hi_f likewise.
 *
 * The device works in three kernels (lfd_amd/csrc/preview/k_preview.h).  k_preview_bin streams the frames once, 4 B per pixel
 * in and 8 B per cell out: a wavefront owns b rows of 256 columns, a lane four neighbouring pixels of each row, which it loads
 * with one 16 B access when every row of the frames starts on a 16 B boundary (the frames' address and W are multiples of 16 B
 * and of 4) and with 4 B accesses otherwise (no unaligned pointer is cast to a wider type); the byte swap and the row flip are in
 * the load and in its address; the lane keeps the b rows' sums in registers, and lanes that share a cell (b = 8, 16) add theirs
 * by shuffles.  k_preview_limits, a workgroup per frame, counts M and selects the two ranks by eight radix passes of 8 bits over
 * the sign-flipped cells, from the top, with histograms in LDS (integer atomics; a wavefront whose cells share a bucket adds
 * once); the two ranks share a histogram until their prefixes part.  k_preview_render keeps lut in LDS and writes a byte per
 * thread, neighbouring threads neighbouring bytes.  The cell plane of a call is made in chunks of frames: max(1, cell_bytes /
 * (8 Hp Wp)) frames (cell_bytes: 1 GiB), and host frames are staged max(1, stage_bytes / (4 H W)) at a time (1 GiB);
 * lfdmi_debug_unit_limits lowers both and lfdmi_debug_unit_split's out[0] counts the chunks.  One frame alone always fits.  What
 * bounds each kernel has not been measured (profiles/preview_probe.txt has the whole call against a copy). */
enum { LFDMI_PREVIEW_RANK = 0, LFDMI_PREVIEW_GIVEN = 1 };
enum { LFDMI_PREVIEW_OK = 0, LFDMI_PREVIEW_FLAT = 1, LFDMI_PREVIEW_EMPTY = 2 };
#define LFDMI_PREVIEW_LUT 4096         /* entries of the stretch table */
typedef struct {
    int32_t bin;              /* 1, 2, 4, 8 or 16; default 4 */
    int32_t mode;             /* LFDMI_PREVIEW_RANK (default) or LFDMI_PREVIEW_GIVEN */
    int32_t lo_ppm, hi_ppm;   /* the two ranks in parts per million of M-1 (0 .. 1000000, lo_ppm <= hi_ppm); defaults 10000, 995000 */
} lfdmi_preview_params;
typedef struct {
    int32_t status;           /* LFDMI_PREVIEW_* */
    int32_t n_cells;          /* M */
    int32_t n_empty;
    int32_t pad;
    int64_t lo, hi;           /* step 4 */
    double lo_f, hi_f;        /* lo, hi times 2^-30: in the frames' units */
} lfdmi_preview_frame;
void lfdmi_default_preview_params(lfdmi_preview_params *out);
/* frames: n frames of h x w, LFDMI_F32 or LFDMI_F32_BE, at loc (host, pinned or device); only read.  p NULL: the defaults.
 * limits: 2 n doubles (host), read in GIVEN mode only.  lut: LFDMI_PREVIEW_LUT bytes (host).  out: n x Hp x Wp uint8 at out_loc
 * (LFDMI_HOST / LFDMI_HOST_PINNED / LFDMI_DEVICE: a caller can preview a whole chunk and fetch the few frames it wants).  cells:
 * NULL, or n x Hp x Wp int64 at out_loc, which get the values m of step 3.  records: n records (host).  n == 0 is a valid call
 * that does nothing.  LFDMI_ERR_ARG, and nothing is written: a bad dtype, loc or out_loc; n < 0; h or w outside 1 .. 65536 or
 * h * w > 1e9; a bad bin or mode; a ppm outside 0 .. 1000000 or lo_ppm > hi_ppm; in GIVEN mode a NULL limits or a limit that is
 * not finite; a NULL lut, and with n > 0 a NULL frames, out or records; calls in flight.  The call keeps no state (its device
 * memory comes from the stream's pool), runs on the context's stream and waits for it once, at its end. */
int lfdmi_frame_previews(lfdmi_ctx *ctx, const void *frames, int dtype, int n, int h, int w, int loc, const lfdmi_preview_params *p,
                         const double *limits, const uint8_t *lut, uint8_t *out, int out_loc, int64_t *cells,
                         lfdmi_preview_frame *records);

#ifdef __cplusplus
}
#endif
#endif
