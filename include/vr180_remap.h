/*
 * vr180_remap.h -- C ABI of the MI355X-native fisheye -> equirectangular remap engine.
 *
 * This is the drop-in boundary for the ONE hot path of 34j/vr180-convert:
 *
 *     apply_lr() -> apply() -> get_map() -> MultiTransformer.transform() -> cv2.remap()
 *     (reference: src/vr180_convert/remapper.py:406,324,23 ; transformer.py:93 ; remapper.py:388-398)
 *
 * The reference has no FFI of its own (it is pure Python over NumPy + OpenCV); what a
 * maintainer would bind is exactly the pair "evaluate the transformer chain on the output
 * grid" + "cv2.remap the image through it".  Every entry point below names the reference
 * lines it replaces.  Plain pointers and sizes only: no torch / numpy / C++ types.
 *
 * All `src`, `dst`, `xmap`, `ymap` pointers are DEVICE pointers (HBM) owned by the caller.
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work
 * on that stream and return without synchronising, except where stated.
 *
 * Return value: 0 on success, a negative V1C_E_* code otherwise; v1c_last_error() returns
 * a thread-local human-readable message for the last failing call on this thread.
 */
#ifndef VR180_REMAP_H
#define VR180_REMAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V1C_ABI_VERSION 1

/* ---- error codes ------------------------------------------------------------------- */
#define V1C_OK             0
#define V1C_E_INVALID     -1   /* bad argument (NULL pointer, size <= 0, unknown enum ...)   */
#define V1C_E_UNSUPPORTED -2   /* valid request the engine cannot lower (caller falls back
                                  to v1c_remap_lut with a map it computed itself)           */
#define V1C_E_HIP         -3   /* a HIP runtime call failed (message has hipGetErrorString)  */
#define V1C_E_NODEVICE    -4   /* no usable gfx950 device                                    */
#define V1C_E_CORRUPT     -5   /* the input data is damaged (v1c_jpeg_decode*)               */

/* ---- cv2 enum values the reference passes straight through ---------------------------
 * remapper.py:330-331 (defaults INTER_LANCZOS4 / BORDER_CONSTANT), cli.py:57-79 (mirrors). */
#define V1C_INTER_NEAREST  0
#define V1C_INTER_LINEAR   1
#define V1C_INTER_CUBIC    2
#define V1C_INTER_AREA     3   /* cv2.remap treats AREA as LINEAR */
#define V1C_INTER_LANCZOS4 4

#define V1C_BORDER_CONSTANT    0
#define V1C_BORDER_REPLICATE   1
#define V1C_BORDER_REFLECT     2
#define V1C_BORDER_WRAP        3
#define V1C_BORDER_REFLECT_101 4
#define V1C_BORDER_TRANSPARENT 5

/* ---- the lowered transformer chain ----------------------------------------------------
 * One v1c_op per stage of the reference's MultiTransformer (transformer.py:87-105), in
 * application order, INCLUDING the NormalizeTransformer that get_map() prepends and the
 * DenormalizeTransformer it appends (remapper.py:51-57).  Stage semantics follow the
 * reference line by line; see DESIGN.md "Op list".                                         */
#define V1C_MAX_OPS    16
#define V1C_MAX_PARAMS 16

enum v1c_opcode {
    /* x=(x-p0)/p2*2 ; y=(y-p1)/p2*2            NormalizeTransformer.transform  transformer.py:153-164
     * optional (nparam = 5): p3 <= row < p4 = the rows of the WHOLE output grid in this plan's row numbering, when the
     * plan serves a band of rows of a larger grid (one eye split over several GPUs): tables sized by the reach of the
     * output are then sized for the whole grid and every band evaluates what the unsplit plan evaluates            */
    V1C_OP_NORMALIZE = 1,
    /* x=x*p0+p2 ; y=y*p1+p3                    DenormalizeTransformer.transform         :197-204 */
    V1C_OP_DENORMALIZE = 2,
    /* x=(x-p2)/p0 ; y=(y-p3)/p1                DenormalizeTransformer.inverse_transform :206-213 */
    V1C_OP_DENORMALIZE_INV = 3,
    /* x=x/p0 ; y=y/p0                          ZoomTransformer.transform                :468-473 */
    V1C_OP_ZOOM = 4,
    /* x=x*p0 ; y=y*p0                          ZoomTransformer.inverse_transform        :475-480 */
    V1C_OP_ZOOM_INV = 5,
    /* iparam = is_latitude_y                   EquirectangularEncoder.transform         :540-568 */
    V1C_OP_EQUIRECT_ENC = 6,
    /* iparam = is_latitude_y                   EquirectangularEncoder.inverse_transform :570-584 */
    V1C_OP_EQUIRECT_DEC = 7,
    /* iparam = v1c_radial kind, nparam/p = its parameters
                                                PolarRollTransformer.transform           :268-286 */
    V1C_OP_RADIAL = 8,
    /* p[0..8] = row-major 3x3 M, v' = M v      Euclidean3DTransformer.transform         :651-657
       (M = numpy-quaternion as_rotation_matrix(q), built by the host: quat.py)                  */
    V1C_OP_ROTATE = 9
};

/* radial function theta' = f(theta) applied by a V1C_OP_RADIAL stage */
enum v1c_radial {
    /* FisheyeEncoder.transform_polar, transformer.py:359-377 */
    V1C_RAD_ENC_RECTILINEAR   = 1,  /* arctan(t)                  */
    V1C_RAD_ENC_STEREOGRAPHIC = 2,  /* 2*arctan(t)                */
    V1C_RAD_ENC_EQUIDISTANT   = 3,  /* t*(pi/2)                   */
    V1C_RAD_ENC_EQUISOLID     = 4,  /* 2*arcsin(t/sqrt(2))        */
    V1C_RAD_ENC_ORTHOGRAPHIC  = 5,  /* arcsin(t)                  */
    /* FisheyeEncoder.inverse_transform_polar (= FisheyeDecoder), transformer.py:379-397 */
    V1C_RAD_DEC_RECTILINEAR   = 6,  /* tan(t)                     */
    V1C_RAD_DEC_STEREOGRAPHIC = 7,  /* 2*tan(t/2)                 */
    V1C_RAD_DEC_EQUIDISTANT   = 8,  /* t/(pi/2)                   */
    V1C_RAD_DEC_EQUISOLID     = 9,  /* sqrt(2)*sin(t/2)           */
    V1C_RAD_DEC_ORTHOGRAPHIC  = 10, /* sin(t)                     */
    /* PolynomialScaler.transform_polar, transformer.py:448-451: p[0..nparam) = coefs_reverse
       (lowest order first); Horner from the highest, starting at 0 like np.polyval.              */
    V1C_RAD_POLYNOMIAL        = 11,
    /* RectilinearDecoder.transform_polar / inverse_transform_polar, transformer.py:338-347,
       p[0] = factor = 2*focal_length/sensor_width_mm                                             */
    V1C_RAD_RECTDEC_FWD       = 12, /* tan(t)*p0                  */
    V1C_RAD_RECTDEC_INV       = 13  /* arctan(t/p0)               */
};

typedef struct v1c_op {
    int32_t opcode;               /* enum v1c_opcode */
    int32_t iparam;               /* integer parameter (kind / flag) */
    int32_t nparam;               /* number of valid entries in p */
    int32_t reserved;
    double  p[V1C_MAX_PARAMS];
} v1c_op;

typedef struct v1c_chain {
    int32_t n_ops;
    int32_t reserved;
    v1c_op  ops[V1C_MAX_OPS];
} v1c_chain;

/* One independent unit of work: an eye of a frame.  remapper.py:388-398 iterates these as
 * `for img in images`; apply_lr concatenates two of them (remapper.py:517-518), which the
 * engine does in place by pointing `dst` at each half of the SBS buffer with dst_pitch = row
 * bytes of the whole SBS image.                                                             */
typedef struct v1c_unit {
    const uint8_t* src;           /* (src_h, src_w, cn) uint8, row pitch src_pitch bytes */
    uint8_t*       dst;           /* (dst_h, dst_w, cn) uint8, row pitch dst_pitch bytes */
    int64_t        src_pitch;
    int64_t        dst_pitch;
    /* optional per-unit rotation (row-major 3x3) REPLACING the matrix of the chain's first
       V1C_OP_ROTATE stage; ignored unless has_rot != 0.  BASELINE config 5: per-frame, per-eye
       calibration rotations (cli.py:308-319) share every other chain parameter.              */
    double         rot[9];
    int32_t        has_rot;
    int32_t        reserved;
} v1c_unit;

typedef struct v1c_plan v1c_plan;   /* opaque */

/* ---- entry points -------------------------------------------------------------------- */

/* ABI / build identification. */
int v1c_abi_version(void);
/* Number of visible HIP devices (<0 on error). Does not create a context. */
int v1c_device_count(void);
/* Thread-local message of the last failing call ("" if none). */
const char* v1c_last_error(void);

/* NUMERICAL CONTRACT of every entry point that evaluates a chain: coordinates in float64, cast to float32 like remapper.py:58; the
 * 1/32-pixel buckets cv2.remap derives from them equal the reference's, pixels equal the CPU oracle's byte for byte -- except at
 * pixels where the CHAIN is ill-conditioned (a map coordinate moving by >= 1e6 x the perturbation of the output position: the pole of
 * a rectilinear projection, stacked polynomials taking an angle to 1e12 rad): there the last bit of the platform's sin / cos / atan2
 * decides the bucket.  BORDER_CONSTANT / BORDER_TRANSPARENT outputs are unaffected (such coordinates lie 1e6+ px outside the source);
 * under the four source-reading border modes those pixels may differ from the reference's.  (And a coordinate whose exact value is
 * a tie of the float64 -> float32 rounding to within a few ulps can land in the neighbouring bucket: measure zero, seen once in 30 000
 * random chains.)  INTEGRATION.md section 2.                                                                                  */

/* Build a reusable plan for one (chain, geometry, interpolation, border) combination.
 * Replaces: chain construction + np.meshgrid + MultiTransformer.transform + astype(float32)
 * of get_map() (remapper.py:50-58) -- here nothing is materialised: the plan only holds the
 * O(W+H) separable tables and the O(1 KiB..32 KiB) radial table the fused kernel reads.
 * `chain` must start with the stage get_map prepends and end with the stage it appends.
 * Synchronous (uploads tables); not graph-capturable.  cn must be 1, 3 or 4.               */
int v1c_plan_create(v1c_plan** out, int device, const v1c_chain* chain,
                    int src_h, int src_w, int dst_h, int dst_w, int cn,
                    int interp, int border_mode, const uint8_t border_val[4]);

/* ---- pixel types: cv2 depth codes -----------------------------------------------------
 * The reference hands whatever array it has to cv2.remap (remapper.py:366-378, 448-456), which takes CV_16U and CV_32F images as well
 * as 8-bit ones: 16-bit TIFF / PNG from RAW development, linear-light float32.  Every entry point without `_ex` is 8-bit.       */
#define V1C_DEPTH_8U  0
#define V1C_DEPTH_16U 2
#define V1C_DEPTH_32F 5

/* v1c_plan_create for any of the depths above.  `border_val` is cv2's Scalar of doubles (NULL = 0), saturated to the pixel type
 * inside (cvRound half to even and [0, 255] / [0, 65535] for 8U / 16U, (float) for 32F).  With V1C_DEPTH_8U it is exactly the plan
 * v1c_plan_create makes.  Plans of a wide depth (16U, 32F) take units whose pointers and pitches are multiples of the pixel type's
 * size, pitches in BYTES (>= w * cn * sizeof); v1c_plan_run serves them through k_remap_wide (V1C_LAUNCH_WIDE, | V1C_LAUNCH_FIXUP
 * behind a fix-up pass), v1c_plan_run_auto / _auto_images return V1C_E_UNSUPPORTED (take the radius to the host), v1c_plan_get_map
 * works as for every plan.  Arithmetic: INTEGRATION.md, "16-bit and float32 images" (cv2's float-weight remap, restated).       */
int v1c_plan_create_ex(v1c_plan** out, int device, const v1c_chain* chain, int src_h, int src_w,
                       int dst_h, int dst_w, int cn, int depth, int interp, int border_mode,
                       const double border_val[4]);
int v1c_plan_destroy(v1c_plan* plan);

/* Which device code path the plan selected: 0 = generic fp64 interpreter, 1 = fused
 * "ray" path (separable tables + radial table), 2 = fused "planar" path.  For tests/bench. */
int v1c_plan_path(const v1c_plan* plan);

/* Enqueue the fused chain+gather for n_units independent units: ONE launch for up to 256 units
 * (longer arrays: one launch per 256; 16 per launch where a fix-up pass or the generic kernels
 * are needed).  Replaces: get_map() + the cv.remap list comprehension, remapper.py:381-398, and
 * the SBS concatenate of apply_lr, remapper.py:517-518 (via dst/dst_pitch).
 * `units` is a HOST array, read before the call returns: up to 16 units travel in the launch's
 * kernel arguments; longer batches are copied into a slot of a plan-owned device ring by small
 * launches on `stream` in front of the remap launch.  The call is launch-only (no allocation,
 * no sync) and may be recorded into a graph (at most 4 recorded launches of more than 16 units
 * per plan: each keeps its ring slot).  One plan may be run from several threads / streams.   */
int v1c_plan_run(v1c_plan* plan, void* stream, const v1c_unit* units, int n_units);

/* v1c_plan_run with the radius read from DEVICE memory: radius="auto" -- the reference's default, remapper.py:333,416 -- without a host
 * round trip or a plan per image.  Replaces get_radius_smart("auto") (remapper.py:82-84: the max over the images of get_radius) feeding
 * get_map's DenormalizeTransformer(scale=(radius, radius)) (remapper.py:51-57).  `rad_dev`: n_rad (radius, status) pairs in device memory as
 * v1c_get_radius_async writes them; the launch uses max(radius) -- clamped to 4 x the larger source dimension in magnitude (a radius
 * beyond that gives the output of the clamped one); if any status is set (the reference raises IndexError there) the scale becomes 0 and
 * the centre (-40000, -40000): every pixel samples the source there under the plan's border mode -- BORDER_CONSTANT the border colour,
 * BORDER_TRANSPARENT leaves the destination untouched, BORDER_REPLICATE / REFLECT / WRAP / REFLECT_101 what those modes read at
 * (-40000, -40000).  The plan's own radius is ignored, so one plan serves every image of a stream; its Denormalize scale must be
 * isotropic (rx == ry, what get_map builds), the launch writes (r, r).  At most 16 units; chains EquirectangularEncoder() * [one
 * rotation] * radial stages whose table needs no fix-up pass -- anything else returns V1C_E_UNSUPPORTED before anything is launched,
 * and the caller takes the radius to the host (v1c_get_radius).  Launch-only,
 * graph-capturable; one plan may be used from several streams (ordered by an event).                                              */
int v1c_plan_run_auto(v1c_plan* plan, void* stream, const v1c_unit* units, int n_units,
                      const double* rad_dev, int n_rad);

/* The same with the estimates taken from the units' OWN source images by the call itself: apply()'s
 * get_radius_smart("auto", images) over the images it is about to remap (remapper.py:379-380;
 * get_radius, transformer.py:108-140, `threshold` its parameter: the reference's default is 10).
 * Two launches in all: one workgroup scans the centre line of every unit's source and sets the
 * scale, then the remap.  Same chains, limits and error behaviour as v1c_plan_run_auto.          */
int v1c_plan_run_auto_images(v1c_plan* plan, void* stream, const v1c_unit* units, int n_units,
                             int threshold);

/* Hand the plan's capture-owned unit buffers out again (see v1c_plan_run: a recorded launch of more
 * than 16 units keeps one of 4 for the graph that replays it).  Call it once every graph that
 * recorded such a launch of this plan has been destroyed -- a process that re-captures over and
 * over (a resolution that changes back and forth) would otherwise get V1C_E_UNSUPPORTED from the
 * 5th such capture on.  Nothing in the reference corresponds to it (no graphs there).             */
int v1c_plan_release_captures(v1c_plan* plan);

/* Which kernels the most recent launch group of v1c_plan_run on this plan used: one of the V1C_LAUNCH_* values, | V1C_LAUNCH_FIXUP
 * when a fix-up pass followed; -1 before the first run.  The engine has several code paths for the same bytes (a generic per-pixel
 * kernel for everything, LDS-tiled kernels for what the plan could prove about the chain and the units); tests use this to make
 * sure a case meant for a tiled kernel was not served by the generic one.  For tests / bench.                                  */
enum {
    V1C_LAUNCH_GENERIC = 0, /* k_remap: fp64 interpreter or the ray path per pixel, samples from global memory */
    V1C_LAUNCH_TILE = 1,    /* BGR, the general tile kernel: k_ray_lin3_tile (pairs, bicubic / Lanczos4, NEAREST, odd cases) */
    V1C_LAUNCH_MIRROR = 2,  /* BGR pairs and single images of unrotated chains: k_ray_lin3_pair_mirror_seq / _raw */
    V1C_LAUNCH_CN = 3,      /* grayscale / BGRA with plan-time boxes: k_ray_lin_cn */
    V1C_LAUNCH_CN_ROT = 4,  /* grayscale / BGRA, units with a rotation of their own: k_ray_lin_cn without boxes */
    V1C_LAUNCH_BATCH = 5,   /* BGR bilinear batches sharing a map: k_ray_lin3_batch_lean_raw (+ k_ray_lin3_tile for its rest tiles) */
    V1C_LAUNCH_ROT_PAIR = 6, /* BGR bilinear units with a rotation of their own: k_ray_lin3_rot_pair_raw */
    V1C_LAUNCH_WIDE = 7,    /* 16-bit / float32 pixels: k_remap_wide (plans of v1c_plan_create_ex with a wide depth) */
    V1C_LAUNCH_CHROMA = 8,  /* BGR, one map per colour channel: k_remap_ca (plans of v1c_ca_plan_create; samples from global memory) */
    V1C_LAUNCH_FIXUP = 0x100
};
int v1c_plan_last_launch(const v1c_plan* plan);

/* Bytes of the plan's tap table, 0 when it holds none.  Plans of BGR bilinear pairs of an unrotated chain whose every tile pair the
 * mirror kernel serves keep the fixed-point tap coordinates of every output pixel, per 4 pixels of the upper half of the image 12
 * bytes, or 8 (the compact entry) where 12 would make a table of more than 8 MiB, computed once at creation by the kernel's own
 * coordinate code; their launches read them instead of evaluating the map.  The size reported is the size allocated.
 * Plans whose table would pass 64 MB, or whose map does not fit the entry format somewhere, hold none and evaluate the map in every
 * launch: the same bytes either way.  For tests / bench and for callers that budget device memory.                              */
int64_t v1c_plan_tap_table_bytes(const v1c_plan* plan);
/* Bytes per entry of that table (12 or 8); 0 when the plan holds none. */
int v1c_plan_tap_entry_bytes(const v1c_plan* plan);

/* Evaluate only the coordinate chain on the output grid and store float32 maps (device
 * pointers, row pitch map_pitch bytes).  Replaces get_map(), remapper.py:23-59.  Used for
 * coordinate-parity tests and for callers that want the map itself.                         */
int v1c_plan_get_map(v1c_plan* plan, void* stream, float* xmap, float* ymap,
                     int64_t map_pitch, const double* rot_or_null);

/* One-shot convenience: plan lookup/creation in an internal cache keyed on every argument
 * but the pointers (the 32 most recently used plans are kept; an evicted plan is destroyed once
 * no call uses it any more), then v1c_plan_run on one unit.  Same replacement as above.       */
int v1c_remap_fused(int device, void* stream,
                    const uint8_t* src, int src_h, int src_w, int64_t src_pitch, int cn,
                    uint8_t* dst, int dst_h, int dst_w, int64_t dst_pitch,
                    const v1c_chain* chain, int interp, int border_mode,
                    const uint8_t border_val[4]);

/* Number of plans the one-shot cache of v1c_remap_fused holds right now (<= 32).  For tests. */
int v1c_fused_cache_size(void);

/* cv2.remap with caller-supplied float32 maps (device pointers).  Replaces the cv.remap call
 * itself, remapper.py:388-398, for transformer chains the engine cannot lower (user-defined
 * TransformerBase subclasses, README.md:204-219): the caller evaluates the chain.           */
int v1c_remap_lut(int device, void* stream,
                  const uint8_t* src, int src_h, int src_w, int64_t src_pitch, int cn,
                  uint8_t* dst, int dst_h, int dst_w, int64_t dst_pitch,
                  const float* xmap, const float* ymap, int64_t map_pitch,
                  int interp, int border_mode, const uint8_t border_val[4]);

/* v1c_remap_lut for any depth (V1C_DEPTH_*): pitches in bytes, `border_val` a cv2 Scalar of doubles as in v1c_plan_create_ex.
 * Wide depths need pointers and pitches that are multiples of the pixel type's size.                                         */
int v1c_remap_lut_ex(int device, void* stream, const void* src, int src_h, int src_w, int64_t src_pitch,
                     int cn, int depth, void* dst, int dst_h, int dst_w, int64_t dst_pitch,
                     const float* xmap, const float* ymap, int64_t map_pitch,
                     int interp, int border_mode, const double border_val[4]);

/* Auto-radius estimate of one device-resident image, get_radius() transformer.py:108-140
 * (centre row / column scan on the device, threshold on the channel mean, sign quirk preserved).
 * Synchronous: returns the value through *radius.  Returns V1C_E_INVALID with the message
 * "no black border" where the reference raises IndexError.                                  */
int v1c_get_radius(int device, void* stream, const uint8_t* img, int h, int w,
                   int64_t pitch, int cn, int threshold, double* radius);
/* The same scan with the result left on the device and nothing synchronised (graph-capturable):
 * out_dev[0] = the radius, out_dev[1] = 0.0 -- or out_dev[0] = NaN, out_dev[1] = 1.0 where the
 * reference raises IndexError.  `out_dev`: two doubles in device (or mapped host) memory.  The
 * scan itself (both forms) is one small kernel: transformer.py:125-140 never leaves the GPU.  */
int v1c_get_radius_async(int device, void* stream, const uint8_t* img, int h, int w,
                         int64_t pitch, int cn, int threshold, double* out_dev);

/* merge=True of apply_lr(), remapper.py:485-497: red/cyan anaglyph of two remapped eyes, both
 * (h, w, 3) uint8 on the device; `out` is (h, w, 3) float64 with row pitch out_pitch BYTES:
 *   out[c] = (mean_L * colL[c] + mean_R * colR[c]) / 255,  colL = (0,128,255), colR = (255,128,0),
 *   mean = float64 mean of the 3 channels -- the reference's NumPy float64 expression, operation
 * by operation (no FMA contraction).  The cv.putText labels (:498-516) stay with the caller.   */
int v1c_anaglyph(int device, void* stream,
                 const uint8_t* left, int64_t left_pitch, const uint8_t* right, int64_t right_pitch,
                 int h, int w, double* out, int64_t out_pitch);

/* The int16 fixed-point weight table the engine uses for INTER_CUBIC (1024*4*4 entries) or
 * INTER_LANCZOS4 (1024*8*8 entries), laid out [fy*32+fx][ky][kx]: OpenCV's initInterTab2D
 * (SURVEY.md Appendix A item 3).  Host-only (no device needed); `out` is a HOST buffer.
 * Lets callers and tests inspect exactly what the kernels read.                            */
int v1c_build_itab(int interp, int16_t* out);

/* The float32 weight table of the 16-bit / float32 sampler: wf[fy*32+fx][ky][kx] = t1d[fy][ky] * t1d[fx][kx] with OpenCV's 1-D
 * weights t1d (the ones v1c_build_itab rounds; LINEAR: {1 - k/32, k/32}) and no sum fix-up.  INTER_LINEAR (1024*2*2 entries),
 * INTER_CUBIC (1024*4*4) or INTER_LANCZOS4 (1024*8*8).  Host-only; `out` is a HOST buffer.                                 */
int v1c_build_ftab(int interp, float* out);

/* ---- feature matching of the two eyes (--automatch devfm; replaces the cv2.AKAZE + BFMatcher front end of remapper.py:194-248) --
 * NOT AKAZE: a single-scale, oriented binary-feature pipeline whose every stage is integer arithmetic, so that its keypoints,
 * descriptors and matches are reproducible bit for bit (INTEGRATION.md section 5 states the contract; tests/feat_ref.py restates it).
 * Defaults in brackets.  `radius` must be positive: get_radius_smart("auto") is negative on an image circle on black (the reference's
 * sign quirk: the 180-degree flip of a map); the qualifying disc is symmetric, and the Python layer passes |radius|.               */
typedef struct v1c_feat_params {
    double  scale;          /* working scale s in (0, 1]: working size (int(w * s), int(h * s)), block-mean resampling [1]      */
    double  radius;         /* image-circle radius in ORIGINAL pixels (what get_radius_smart resolves), centre (w / 2, h / 2)   */
    int32_t fast_threshold; /* FAST-9 score threshold, 1..255 [20]                                                             */
    int32_t margin;         /* keypoints lie within radius * s - margin working pixels of the centre [19]                      */
    int32_t cell;           /* grid cell in working pixels, 8..64 [32]                                                         */
    int32_t per_cell;       /* keypoints kept per cell, 1..4 [2]                                                                */
    int32_t max_keypoints;  /* N_max, 1..2^20 [8192]: the capacity of kp_out / desc_out                                          */
    int32_t max_distance;   /* match: largest Hamming distance kept, 0..256 [64]                                                 */
    int32_t ratio_num;      /* match: kept iff ratio_den * d1 <= ratio_num * d2 [3 / 4]                                          */
    int32_t ratio_den;
} v1c_feat_params;

typedef struct v1c_feat_kp {
    int32_t x, y;           /* working-scale pixel                                                                              */
    int32_t score;          /* FAST-9 score                                                                                     */
    int32_t bin;            /* orientation sector 0..29 (12 degrees each)                                                       */
    int32_t src_x2, src_y2; /* twice the centre of the keypoint's source block in original pixels: c0 + c1 - 1, r0 + r1 - 1       */
} v1c_feat_kp;

/* Keypoints and 32-byte descriptors of one uint8 image (device pointer, (h, w, cn), cn 1 / 3 / 4, BGR(A) order).  Writes at most
 * max_keypoints records to kp_out and descriptors to desc_out (device; desc_out 8-byte aligned), cell-major, and their number to
 * *count_out_dev (device).  Enqueues its work on `stream` (scratch allocated stream-ordered) and waits for none of it, with two host-side
 * exceptions: the first call on a device uploads the sampling pattern with a blocking copy, and every call copies its host-computed
 * tables (block boundaries, qualifying columns per row: 4 (w' + h') + 8 h' bytes) from pageable memory, a copy that HIP may
 * finish before returning.  Rows and columns within 16 working pixels of the image edge never hold a keypoint, whatever the radius
 * and the margin.  V1C_E_INVALID for cn outside
 * {1, 3, 4}, s outside (0, 1], a working image smaller than 33 x 33, an empty circle, NULL pointers, parameters out of range.     */
int v1c_feat_detect(int device, void* stream, const uint8_t* img, int h, int w, int64_t pitch, int cn,
                    const v1c_feat_params* params, v1c_feat_kp* kp_out, uint8_t* desc_out, int32_t* count_out_dev);

/* Brute-force Hamming match of n_a descriptors against n_b (device, 16-byte aligned), both directions.  Pair (i, j) is kept iff i and j
 * are each other's best (ties: the lowest index), d1 <= max_distance and ratio_den * d1 <= ratio_num * d2 (d2: the second-best
 * distance of i's row; with a single candidate only the max_distance test applies).  pairs_out (i, j) int32 pairs and dist_out in
 * query order, at most min(n_a, n_b); their number to *count_out_dev.  Launch-only.                                              */
int v1c_feat_match(int device, void* stream, const uint8_t* desc_a, int n_a, const uint8_t* desc_b, int n_b,
                   const v1c_feat_params* params, int32_t* pairs_out, int32_t* dist_out, int32_t* count_out_dev);

/* The rotated sampling pattern the descriptors read: 30 sectors x 256 pairs x (px, py, qx, qy) int8 offsets (30 720 bytes).
 * Host-only; `out` is a HOST buffer.                                                                                            */
int v1c_feat_pattern(int8_t* out);

/* ---- the image circle from its rim (INTEGRATION.md section 11 states the contract; tests/circle_ref.py restates it) ---------------
 * A pixel is LIT when the sum of its channels is >= threshold * cn (the integer complement of get_radius's mean < threshold, alpha
 * included).  RIM POINTS: from each end of every row, then of every column, the first pixel of the first run of at least `run` lit
 * pixels; a point on the frame's own first / last column (row, for columns) is dropped.  FIT: Kasa's algebraic circle from the int64
 * moment sums of the points (coordinates relative to (w / 2, h / 2)), solved in float64, then `rounds` refits, round k over the points
 * whose distance from the centre of the fit before it lies within tol16[k] / 16 px of its radius -- centre and radius rounded to
 * 1/16 px (half up), the comparison made on the squares in int64.  The result is a pure function of the pixels and the parameters.
 * RESULT, eight doubles: cx, cy, r (source pixels, r > 0), status, n_rim, n_used, rms, 0.  status: 0, or 1 (fewer than min_points
 * points in a fit), 2 (singular system), 3 (r <= 0, r > 4 max(h, w), or a centre further than 8 max(h, w) from the frame's); then
 * cx = cy = r = rms = 0.  n_used: the points of the last fit made; rms: sqrt(mean((floor(d16) - r16)^2)) / 16 over them, d16 the
 * distance from the final centre in 1/16 px.  An all-black or all-lit image ends in status 1, not in an error.                  */
typedef struct v1c_circle_params {
    int32_t threshold;      /* 0..65535 [10]                                                                                     */
    int32_t run;            /* 1..64 [4]: isolated lit pixels shorter than this are no rim                                       */
    int32_t rounds;         /* trimmed refits, 0..8 [4]                                                                          */
    int32_t min_points;     /* 3..2^20 [8]                                                                                       */
    int32_t tol16[8];       /* tolerance of round k in 1/16 px, 1..2^20 [128, 48, 24, 24]                                        */
} v1c_circle_params;

typedef struct v1c_circle_point {
    int32_t x, y;           /* source pixel                                                                                      */
    int32_t selected;       /* 1: in the last selection made                                                                     */
} v1c_circle_point;

/* Bytes of device memory a fit of an (h, w) image needs as its workspace: 2 (h + w) point slots, their flags, the result of the
 * synchronous form and one record per column and band of 64 rows.  Host-only.  0 for sizes outside 1..32768.                    */
uint64_t v1c_fit_circle_workspace(int h, int w);

/* Fits the circle of the device image img ((h, w, cn), cn 1 / 3 / 4, depth V1C_DEPTH_8U or _16U, row pitch in BYTES) on `stream`:
 * four launches, no allocation, no copy, no synchronisation -- it can be captured into a graph.  `workspace`: device memory of
 * v1c_fit_circle_workspace(h, w) bytes, 4-byte aligned, the caller's, in use until the work has run (one per call in flight);
 * out_dev8: eight doubles on the device.  params NULL: the defaults.  V1C_E_INVALID before any device call for NULL pointers, cn,
 * depth, sizes, pitch below a row's bytes, an odd pointer or pitch of a 16-bit image, alignment, parameters out of range.       */
int v1c_fit_circle_async(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int depth,
                         const v1c_circle_params* params, void* workspace, double* out_dev8);

/* The same, SYNCHRONISES the stream once and leaves the eight doubles in out_host8 (HOST).  points_out (HOST, may be NULL): the rim
 * points in order -- by row (left, right), then by column (top, bottom) -- at most `capacity`, their number in *n_points_out
 * (V1C_E_INVALID after the fact when there are more; 2 (h + w) always suffices).  V1C_E_UNSUPPORTED while `stream` is captured.   */
int v1c_fit_circle(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int depth,
                   const v1c_circle_params* params, void* workspace, double* out_host8, v1c_circle_point* points_out,
                   int32_t capacity, int32_t* n_points_out);

/* ---- the colours of one eye matched to the other's (INTEGRATION.md section 12 states the contract; tests/colormatch_ref.py restates
 * it).  Two (h, w, cn) 8-bit device images of one shape, cn 1 / 3 / 4, each with its own row pitch in BYTES.  MASK: a position counts
 * when the maximum over the colour channels (the first three of four, or the only one) lies in [lo, hi] in BOTH eyes; n positions
 * count.  HISTOGRAMS: h[eye][c][v], uint32, eye 0 = left, over the counted positions.  The TARGET is the eye that is not the
 * reference; T, R are the target's and the reference's counts of one channel, CT, CR their running sums.
 * MODE HISTOGRAM: knots (v, min{u : 2 CR[u] >= CT[v-1] + CT[v]}) at every populated bin v of T, (0, 0) and (255, 255) where bin 0 /
 * 255 is not populated; between neighbouring knots (a, ma), (b, mb): m = ma + ((v-a)(mb-ma) 2 + (b-a)) / (2 (b-a)), floored; the entry
 * is clamp(clamp(m, v - max_shift, v + max_shift), 0, 255).  MODE GAIN: sT, sR the sums of v T[v], v R[v] (int64),
 * g = clamp((sR 65536 + sT / 2) / sT, 16384, 262144), the entry min(255, (v g + 32768) >> 16).
 * REPORT, 20 int32: status, n, then per colour channel c at 2 + 5 c: first and last populated bin of the left eye, of the right eye
 * (-1: none, or a channel the image lacks), g (0 outside gain mode and where sT is 0); two spare words, 0.  status: 0, or 1
 * (n < min_pixels), 2 (gain mode, sT == 0 in a channel; 1 goes first).  A non-zero status gives identity tables.  A one-channel
 * image's second and third table are the identity.                                                                              */
#define V1C_CM_MODE_HISTOGRAM   0
#define V1C_CM_MODE_GAIN        1
#define V1C_CM_REFERENCE_LEFT   0
#define V1C_CM_REFERENCE_RIGHT  1

typedef struct v1c_color_match_params {
    int32_t mode;           /* V1C_CM_MODE_* [HISTOGRAM]                                                                         */
    int32_t reference;      /* V1C_CM_REFERENCE_* [LEFT]: the eye that stays as it is                                            */
    int32_t lo, hi;         /* the mask, 0 <= lo <= hi <= 255 [10, 254]                                                          */
    int32_t max_shift;      /* 0..255 [64]                                                                                       */
    int32_t min_pixels;     /* >= 0 [1024]                                                                                       */
} v1c_color_match_params;

/* Bytes of device memory v1c_color_match_luts_async needs as its workspace (the histograms: 2 x 3 x 256 uint32).  Host-only.       */
uint64_t v1c_color_match_workspace(void);

/* Builds the three 256-entry tables that map the target eye onto the reference eye, on `stream`: the workspace zeroed, two launches,
 * no allocation, no copy to the host, no synchronisation -- it can be captured into a graph, and a replay starts from a zeroed
 * workspace.  `workspace`: device memory of v1c_color_match_workspace() bytes, 4-byte aligned, the caller's, in use until the work has
 * run; it holds the histograms afterwards.  luts_dev: 3 x 256 bytes, report_dev: 20 int32, both on the device.  params NULL: the
 * defaults.  Neither eye is written.  V1C_E_INVALID before any device call for NULL pointers, cn, non-positive sizes or
 * h * w >= 2^31, a pitch below a row's bytes, alignment, parameters out of range.                                                 */
int v1c_color_match_luts_async(int device, void* stream, const void* left, int64_t left_pitch, const void* right, int64_t right_pitch,
                               int h, int w, int cn, const v1c_color_match_params* params, void* workspace, uint8_t* luts_dev,
                               int32_t* report_dev);

/* dst[c] = luts[c][src[c]] on the colour channels of an (h, w, cn) 8-bit device image, a fourth channel copied; one launch on `stream`.
 * dst may be src (in place) or another image that does not overlap it, with its own pitch.  The tables may come from another pair of
 * the same shoot.  V1C_E_INVALID as above.                                                                                        */
int v1c_apply_luts_async(int device, void* stream, const void* src, int64_t src_pitch, void* dst, int64_t dst_pitch, int h, int w, int cn,
                         const uint8_t* luts_dev);

/* ---- Lens vignetting: a radial gain over the image circle (INTEGRATION.md section 14 states the contract; tests/vignette_ref.py
 * restates it).  Integer arithmetic from end to end; the only floating-point step is the host's sampling of the gain curve into the
 * tables.  For the pixel (x, y) of an (h, w, cn) image of 8- or 16-bit elements (elem_bytes 1 / 2, maxv 255 / 65535):
 *   r2  = (x - cx)^2 + (y - cy)^2, exact, in 64 bits                  (below 2^34: h, w <= 32767, -w <= cx < 2 w, -h <= cy < 2 h)
 *   q   = (r2 * scale) >> shift, in unsigned 64 bits                   (0 < scale < 2^30, 0 <= shift <= 62)
 *   idx = q >> 8, f = q & 255; where q >> 8 >= 1024: idx = 1023, f = 255 (the last interval is held)
 *   G   = (T[idx] (256 - f) + T[idx + 1] f + 128) >> 8                (T: the channel's table, 1025 uint16 in Q14)
 *   out = min(maxv, (v G + 2^13) >> 14)
 * TABLES: 3 x 1025 uint16, in the order of a BGR pixel's channels.  A one-channel image takes the second (green) table; a fourth
 * channel is copied.
 * RINGS: over every pixel with r2 < R2 whose colour channels all lie in [lo, hi], ring = min(rings - 1, (r2 * rings) / R2): the
 * channel's value is added to the ring's sum and 1 to its count.  The record is rings x 4 int64: sumB, sumG, sumR, n; a one-channel
 * image fills sumG only.                                                                                                          */
typedef struct v1c_vignette_geom {
    int32_t cx, cy;         /* the circle's centre, pixels                                                                       */
    uint32_t scale;         /* the table position's multiplier: about 256 * 1024 * 2^shift / radius^2                            */
    int32_t shift;
} v1c_vignette_geom;

typedef struct v1c_vignette_ring_params {
    int32_t cx, cy;         /* the circle's centre, pixels                                                                       */
    int64_t r2;             /* R2: the circle's squared radius, 1 <= r2 < 2^35                                                    */
    int32_t rings;          /* 16..1024, uniform in r2: equal areas                                                              */
    int32_t lo, hi;         /* the mask, 0 <= lo <= hi <= maxv                                                                   */
    int32_t reserved;       /* 0                                                                                                 */
} v1c_vignette_ring_params;

/* The gain pass of an (h, w, cn) device image; one launch on `stream`, no allocation, no copy, no synchronisation -- it can be
 * captured into a graph.  dst may be src (in place) or another image that does not overlap it, with its own pitch.  tables_dev: the
 * 3 x 1025 uint16 tables on the device; they may serve every frame of a shoot.  V1C_E_INVALID before any device call for NULL
 * pointers, cn, elem_bytes, sizes outside 1..32767, a pitch below a row's bytes, pointers or pitches that are no multiple of
 * elem_bytes, a centre further than one frame size outside the frame, scale or shift out of range.                                */
int v1c_vignette_apply_async(int device, void* stream, const void* src, int64_t src_pitch, void* dst, int64_t dst_pitch, int h, int w,
                             int cn, int elem_bytes, const v1c_vignette_geom* geom, const uint16_t* tables_dev);

/* The ring statistics of an (h, w, cn) device image, on `stream`: the record zeroed by a launch, then one launch; no allocation, no
 * copy to the host, no synchronisation -- it can be captured into a graph, and a replay starts from a zeroed record.  rings_dev:
 * params->rings x 4 int64 on the device, 8-byte aligned; the sums are exact whatever the order of the adds.  The image is not written.
 * V1C_E_INVALID as above, and for parameters out of range.                                                                        */
int v1c_vignette_rings_async(int device, void* stream, const void* src, int64_t src_pitch, int h, int w, int cn, int elem_bytes,
                             const v1c_vignette_ring_params* params, int64_t* rings_dev);

/* ---- PNG encoding of a device image (INTEGRATION.md section 6 states the stream; tests/png_ref.py restates it) ------------------
 * The image's filtered scanlines, cut into bands of band_rows rows, every band deflated from an empty window as ONE dynamic Huffman
 * block of literals and distance-1 matches (zlib's Z_RLE class) closed by an empty stored block, or as stored blocks where that is
 * smaller.  The caller wraps the concatenated band segments into a zlib stream and a PNG container (_png.assemble).               */
#define V1C_PNG_FILTER_UP    2
#define V1C_PNG_FILTER_PAETH 4

typedef struct v1c_png_band {
    uint32_t row0, row1;    /* the band's rows [row0, row1)                                                                      */
    uint64_t offset, size;  /* its segment of out_host                                                                           */
    uint32_t adler32;       /* of its scanline bytes                                                                             */
    uint32_t stored;        /* 1: stored blocks, 0: one dynamic block + the empty stored block                                   */
} v1c_png_band;

/* Bytes the band segments of an (h, w, cn) image of `depth` (V1C_DEPTH_8U / _16U) can need: every band as stored blocks (scanline
 * bytes + 5 per started 65535) + 8 per band.  Host-only.  0 for invalid arguments.                                              */
uint64_t v1c_png_bound(int h, int w, int cn, int depth, int band_rows);

/* Encodes the device image img ((h, w, cn) in cv2 channel order, cn 1 / 3 / 4, uint8 or uint16, row pitch in BYTES) on `stream`,
 * SYNCHRONISES the stream (twice: once for the histograms the host builds the codes from, once at the end) and leaves the band
 * segments back to back in out_host (HOST memory of `capacity` >= v1c_png_bound bytes; page-locked recommended), one v1c_png_band
 * per band in bands_out (host, ceil(h / band_rows) records), their number in *n_bands_out and the total in *size_out.  The result
 * is a pure function of the pixels and the parameters.  V1C_E_INVALID before any device call for cn, depth, filter, sizes < 1 or
 * above 2^20, a band above 2^31 - 1 scanline bytes, NULL pointers, capacity below the bound, pitch < row bytes, a 16-bit image
 * whose pointer or pitch is odd.                                                                                                */
int v1c_png_deflate(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int depth, int filter,
                    int band_rows, uint8_t* out_host, uint64_t capacity, v1c_png_band* bands_out, int32_t* n_bands_out,
                    uint64_t* size_out);

/* ---- JPEG encoding of a device image (INTEGRATION.md section 7 states the file; tests/jpg_ref.py restates it) --------------------
 * Baseline sequential DCT (SOF0), 8-bit, JFIF BT.601 YCbCr in 4:2:0 or 4:4:4 (one component for cn = 1; alpha of cn = 4 is dropped),
 * the Annex K quantisation tables scaled by the IJG quality rule, the Annex K Huffman tables, restart intervals of restart_mcus MCUs.
 * A decodable file, not libjpeg's output byte for byte.                                                                           */
#define V1C_JPEG_444 0
#define V1C_JPEG_420 2
#define V1C_JPEG_HEADER_MAX 1024 /* bytes v1c_jpeg_header can write (613 for three components)                                    */

/* Bytes the scan of an (h, w, cn) image can need: every block at its longest (208 bytes), one pad byte per interval, every byte
 * stuffed, one marker per interval.  Host-only.  0 for invalid arguments.                                                        */
uint64_t v1c_jpeg_bound(int h, int w, int cn, int subsampling, int restart_mcus);

/* Everything of the file in front of the scan (SOI, APP0, DQT, SOF0, DHT, DRI, SOS) into the HOST buffer `out`; the file is these
 * bytes, the scan of v1c_jpeg_encode and EOI (0xFF 0xD9).  Host-only.  Returns the number of bytes, or V1C_E_INVALID.           */
int64_t v1c_jpeg_header(int h, int w, int cn, int quality, int subsampling, int restart_mcus, uint8_t* out, uint64_t capacity);

/* Encodes the device image img ((h, w, cn) uint8 in cv2 channel order, cn 1 / 3 / 4, row pitch in BYTES; pixels and channels dense)
 * on `stream` and leaves the scan -- the entropy-coded data with its stuffing bytes and RSTm markers -- in out_host (HOST memory of
 * `capacity` >= v1c_jpeg_bound bytes; page-locked recommended) and its size in *size_out.  The kernels form one chain without a
 * host step; the call SYNCHRONISES the stream twice: once for the size, once for the scan.  The result is a pure function of the
 * pixels and the parameters.  V1C_E_INVALID before any device call for cn, quality outside 1 ... 100, subsampling, restart_mcus
 * outside 1 ... 65535, sizes < 1 or above 65535, NULL pointers, capacity below the bound, pitch < row bytes.                     */
int v1c_jpeg_encode(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling,
                    int restart_mcus, uint8_t* out_host, uint64_t capacity, uint64_t* size_out);

/* A list of device images in shared launches: every out_host receives, byte for byte, the scan v1c_jpeg_encode writes for that image
 * and those parameters, and `size` its size.  Size, channels, pitch, quality, subsampling and restart interval are per image.  The
 * images of a chunk share ONE stream-ordered workspace, one upload (descriptors, work lists, one set of tables per distinct
 * quality), one chain of kernels and TWO synchronisations: one for all sizes, one for all scans (one copy of exactly `size` bytes per
 * image).  The list is cut into chunks whose workspaces -- about 760 bytes per 8 x 8 block -- stay within workspace_budget (0: 1 GiB);
 * an image larger than the budget is a chunk of its own; *chunks_out (may be NULL): the chunks that ran.  All arguments of all
 * images are checked with v1c_jpeg_encode's rules before any device call: a bad image makes the whole call V1C_E_INVALID and the
 * message names its index; n < 0 or a NULL array are V1C_E_INVALID, n == 0 returns V1C_OK at once.  The call synchronises inside:
 * V1C_E_UNSUPPORTED, before anything is done, while `stream` is being captured into a graph.                                      */
typedef struct v1c_jpeg_image {       /* one image of a batch; every field as the argument of the same name of v1c_jpeg_encode */
    const void* img;
    int h, w;
    int64_t pitch;
    int cn, quality, subsampling, restart_mcus;
    uint8_t* out_host;
    uint64_t capacity;                /* >= v1c_jpeg_bound of this image                                                        */
    uint64_t size;                    /* out: bytes of its scan                                                                 */
} v1c_jpeg_image;
int v1c_jpeg_encode_batch(int device, void* stream, int n, v1c_jpeg_image* images, uint64_t workspace_budget, uint32_t* chunks_out);

/* ---- Optimised Huffman tables (INTEGRATION.md section 7 states the procedure; tests/jpg_opt_ref.py restates it) -------------------
 * The same file with Huffman tables built for the image -- its symbols are counted on the device, then libjpeg's
 * jpeg_gen_optimal_table procedure runs there on the counts -- in place of the Annex K tables: the same coefficients, a smaller scan
 * and a smaller DHT segment.  The entries above do not change with it.  v1c_jpeg_bound holds for the optimised scan too: a DC table
 * has at most 13 leaves, so a DC code is at most 12 bits and a block at most 23 + 63 * 26 bits, within the 208 bytes of the bound.   */
#define V1C_JPEG_DHT_MAX (4 * (1 + 16 + 256)) /* bytes of the DHT segment's body: per table Tc << 4 | Th, BITS, HUFFVAL            */
#define V1C_JPEG_HEADER_OPT_MAX 2048          /* bytes v1c_jpeg_header_opt can write                                                */

/* v1c_jpeg_header with the DHT body of v1c_jpeg_encode_opt / v1c_jpeg_encode_batch_opt (`dht`, dht_size <= V1C_JPEG_DHT_MAX bytes:
 * the two tables of a cn = 1 image or the four of a colour image) in place of the Annex K tables.  Host-only.  Returns the number
 * of bytes, or V1C_E_INVALID (also for a body that is not whole tables in the segment's order).                                      */
int64_t v1c_jpeg_header_opt(int h, int w, int cn, int quality, int subsampling, int restart_mcus, const uint8_t* dht, uint32_t dht_size,
                            uint8_t* out, uint64_t capacity);

/* v1c_jpeg_encode with optimised tables: the scan in out_host (capacity >= v1c_jpeg_bound), its size in *size_out, and the DHT
 * segment's body in dht_out (HOST memory of V1C_JPEG_DHT_MAX bytes) with its size in *dht_size_out, for v1c_jpeg_header_opt.  The
 * tables are built on the device between two kernels of the chain, and their record comes to the host in the copy of the size: the
 * call SYNCHRONISES the stream twice, as v1c_jpeg_encode does.  Arguments are checked as there; V1C_E_UNSUPPORTED while `stream`
 * is being captured into a graph.                                                                                                   */
int v1c_jpeg_encode_opt(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling,
                        int restart_mcus, uint8_t* out_host, uint64_t capacity, uint64_t* size_out, uint8_t* dht_out,
                        uint32_t* dht_size_out);

/* v1c_jpeg_encode_batch with optimised tables per image: an image with optimize != 0 gets, byte for byte, the scan and the DHT body
 * of v1c_jpeg_encode_opt, one with optimize == 0 the scan of v1c_jpeg_encode (dht_size 0).  The chunk's upload holds one set of
 * tables per distinct quality of the plain images and one per optimising image; every chunk still synchronises TWICE: the records
 * of all its tables come with its sizes.  Everything else as v1c_jpeg_encode_batch.                                               */
typedef struct v1c_jpeg_image_opt {   /* one image of a batch; the fields of v1c_jpeg_image, then:                                */
    const void* img;
    int h, w;
    int64_t pitch;
    int cn, quality, subsampling, restart_mcus;
    uint8_t* out_host;
    uint64_t capacity;
    uint64_t size;
    int optimize;                     /* != 0: tables of its own                                                                 */
    uint32_t dht_size;                /* out: bytes of dht, 0 for optimize == 0                                                  */
    uint8_t dht[V1C_JPEG_DHT_MAX];    /* out: the DHT segment's body                                                             */
} v1c_jpeg_image_opt;
int v1c_jpeg_encode_batch_opt(int device, void* stream, int n, v1c_jpeg_image_opt* images, uint64_t workspace_budget, uint32_t* chunks_out);

/* ---- JPEG decoding into a device image (INTEGRATION.md section 8 states the contract; tests/jpgdec_ref.py restates it) ------------
 * Sequential DCT with Huffman coding and 8-bit samples (SOF0, SOF1) in one interleaved scan: one component, or three as JFIF YCbCr
 * in 4:4:4, 4:2:2 or 4:2:0; any DQT, DHT and DRI.  Everything else a JPEG file may be -- progressive, lossless, arithmetic, 12-bit,
 * several scans, DNL, other sampling factors, four components, Adobe transform 0 -- is V1C_E_UNSUPPORTED from a host-only parse,
 * a damaged file V1C_E_CORRUPT.  The Huffman decoding is parallel over subsequences of the unstuffed scan whose entry states are
 * found by iteration; the pixels follow libjpeg's default decoder (accurate integer IDCT, triangle-filter upsampling).           */
typedef struct v1c_jpeg_info {
    int32_t height, width;
    int32_t components;        /* 1 or 3                                                                                          */
    int32_t h_samp, v_samp;    /* luma sampling factors: 1x1 (grey, 4:4:4), 2x1 (4:2:2), 2x2 (4:2:0)                              */
    int32_t restart_interval;  /* MCUs; 0: none                                                                                   */
} v1c_jpeg_info;

typedef struct v1c_jpeg_decode_report {
    uint32_t segments;         /* stretches of the scan between restart markers                                                   */
    uint32_t subsequences;     /* lanes of the parallel decode                                                                    */
    uint32_t rounds;           /* launches until no subsequence's entry state changed                                             */
    uint32_t reserved;
    uint64_t error_pos;        /* V1C_E_CORRUPT / V1C_E_UNSUPPORTED: byte of the file where the parse stopped, or bit of the
                                  unstuffed scan where decoding did                                                               */
} v1c_jpeg_decode_report;

/* Host-only parse of a file of `size` bytes in HOST memory: the markers and one walk over the scan's 0xFF bytes.  Touches no device.
 * V1C_E_INVALID for NULL pointers, else V1C_OK, V1C_E_UNSUPPORTED or V1C_E_CORRUPT (what a parse can tell; a damaged entropy-coded
 * segment shows only in v1c_jpeg_decode).                                                                                        */
int v1c_jpeg_decode_info(const uint8_t* file, uint64_t size, v1c_jpeg_info* info);

/* Decodes the file into the device image out ((height, width, out_cn) uint8, cv2 channel order, row pitch in BYTES): out_cn 3, or 1
 * for a file of one component (which out_cn 3 replicates).  The scan is uploaded from a page-locked staging buffer on `stream`.
 * subseq_bits: bits of the unstuffed scan one lane decodes -- a multiple of 32, at least 256, 0 for the default; the pixels do not
 * depend on it.  The call SYNCHRONISES the stream once per round and once for the verdict on the stream, and returns with the
 * remaining kernels queued; it cannot be captured into a graph (V1C_E_UNSUPPORTED under capture).  `report` may be NULL.  After
 * V1C_E_CORRUPT the image's content is unspecified.  No read leaves the uploaded data and its padding whatever the file holds.  */
int v1c_jpeg_decode(int device, void* stream, const uint8_t* file, uint64_t size, void* out, int64_t pitch, int out_cn,
                    uint32_t subseq_bits, v1c_jpeg_decode_report* report);

/* v1c_jpeg_decode of n files in shared kernel launches and shared synchronisation rounds: file i of sizes[i] bytes into outs[i] with
 * pitches[i] and out_cns[i].  The pixels, reports[i].segments, .subsequences and .rounds are the single call's, file by file; the call
 * SYNCHRONISES the stream once per round of its SLOWEST file (not once per round of every file) and once for the verdict, per chunk.
 * All files are parsed on the host first.  status[i] is what v1c_jpeg_decode would have returned for the file: V1C_E_INVALID (NULL
 * pointer, out_cn, pitch), V1C_E_UNSUPPORTED or V1C_E_CORRUPT from the parse with reports[i].error_pos the byte -- such a file is left
 * out and the others are decoded -- or V1C_E_CORRUPT from the last pass with error_pos the bit: that file has no pixel stage, so its
 * image's content is unspecified (whatever the buffer held), and every other file's image is exactly its own.
 * max_workspace_bytes: the files are taken in order into chunks whose summed device workspace (about 200 bytes per 8 x 8 block of a
 * file, plus its scan twice) stays within it; 0: 1 GiB; a file above it is a chunk of its own.  Chunks run one after another on the
 * stream, each with one stream-ordered allocation; reports[i].reserved is the file's chunk and *batch_rounds (may be NULL) the round
 * launches of all chunks together: within a chunk the largest of its files' rounds.
 * Returns V1C_OK when it ran (n == 0: at once), V1C_E_INVALID for n < 0, NULL arrays or subseq_bits, V1C_E_UNSUPPORTED under stream
 * capture (before anything is done), V1C_E_NODEVICE / V1C_E_HIP as the single call; then status[] and the images are unspecified.   */
int v1c_jpeg_decode_batch(int device, void* stream, int n, const uint8_t* const* files, const uint64_t* sizes, void* const* outs,
                          const int64_t* pitches, const int* out_cns, uint32_t subseq_bits, uint64_t max_workspace_bytes, int* status,
                          v1c_jpeg_decode_report* reports, uint32_t* batch_rounds);

/* ---- progressive JPEG files ("Progressive files"; tests/jpgprog_ref.py restates the contract) ---------------
 * SOF2 with Huffman coding and 8-bit samples, components and sampling as above, with any legal scan script (ISO/IEC 10918-1 G.1: DC
 * and AC, first and refinement scans, any band and point transform), DHT, DQT and DRI between the scans.  The two calls above keep
 * refusing such a file; these two take nothing else (a sequential file is V1C_E_UNSUPPORTED here).  A script that does not bring every
 * coefficient of every component to full precision is V1C_E_UNSUPPORTED (libjpeg smooths such a file; the contract is the plain
 * decode), an illegal script V1C_E_CORRUPT, both from the host-only parse.  Every scan is decoded as the sequential decoder's one
 * scan is -- subsequences, rounds -- into one coefficient store; the pixel stage behind the last scan is the sequential decoder's. */
typedef struct v1c_jpeg_prog_info_t {
    int32_t height, width;
    int32_t components;        /* 1 or 3                                                                                          */
    int32_t h_samp, v_samp;
    int32_t scans;
    uint64_t error_pos;        /* V1C_E_CORRUPT / V1C_E_UNSUPPORTED: byte of the file where the parse stopped                     */
} v1c_jpeg_prog_info_t;

typedef struct v1c_jpeg_prog_report {
    uint32_t scans;
    uint32_t segments;         /* summed over the scans, as the next two                                                          */
    uint32_t subsequences;
    uint32_t rounds;
    uint32_t error_scan;       /* V1C_E_CORRUPT by the decode: the scan (from 0) ...                                              */
    uint32_t reserved;
    uint64_t error_pos;        /* ... and the bit of its unstuffed bytes; by the parse: the byte of the file                      */
} v1c_jpeg_prog_report;

/* Host-only parse of all the scans of a progressive file in HOST memory.  Touches no device.  V1C_E_INVALID for NULL pointers, else
 * V1C_OK, V1C_E_UNSUPPORTED or V1C_E_CORRUPT.                                                                                    */
int v1c_jpeg_prog_info(const uint8_t* file, uint64_t size, v1c_jpeg_prog_info_t* info);

/* v1c_jpeg_decode for a progressive file: the same arguments with the same meaning and the same order of checks (arguments and the
 * parse before any device call, V1C_E_UNSUPPORTED under stream capture, the device's staging buffer and its lock, one stream-ordered
 * workspace).  The stream is SYNCHRONISED once per round and once for the verdict of EVERY scan.  scan_rounds (may be NULL with
 * scan_cap 0) receives the rounds of the first scan_cap scans.  The earliest damaged scan's smallest bad bit is reported.         */
int v1c_jpeg_prog_decode(int device, void* stream, const uint8_t* file, uint64_t size, void* out, int64_t pitch, int out_cn,
                         uint32_t subseq_bits, v1c_jpeg_prog_report* report, uint32_t* scan_rounds, uint32_t scan_cap);

/* ---- lossless JPEG crop, split and swap (INTEGRATION.md section 9 states the contract; tests/jpgxc_ref.py restates it) ----------------
 * A file that v1c_jpeg_decode_info accepts -- one component, or three in 4:4:4, 4:2:2 or 4:2:0 -- is cut on MCU boundaries in the DCT domain:
 * the entropy decoder of v1c_jpeg_decode runs up to its DC scan, a gather kernel copies rectangles of MCUs into the encoder's
 * coefficient store, and the stages of v1c_jpeg_encode behind its transform code them again.  No coefficient changes, so every sample
 * a reader decodes from the gathered MCUs is the sample it decodes from the source; only the Huffman coding and the restart intervals
 * are the outputs' own.  An output is tiled by regions: a rectangle of nx x ny source MCUs from MCU (src_x, src_y), placed with its
 * first MCU at MCU (dst_x, dst_y) of the output.  An MCU is 8 x 8 pixels (one component, 4:4:4), 16 x 8 (4:2:2) or 16 x 16 (4:2:0).  A crop is one
 * output of one region, a split two outputs of one region each, a swap of the halves one output of two regions.  A region may hold the
 * source's partial last MCU column or row.  An output's width and height are the caller's: its MCU columns and rows are those of that
 * size, and the regions must cover each of them exactly once.
 * V1C_E_UNSUPPORTED from the host-only parse for what v1c_jpeg_decode_info refuses (progressive files among it), for
 * Cb and Cr with different quantisation tables, and for regions that overlap in an output; V1C_E_CORRUPT for a damaged file;
 * V1C_E_INVALID for every other rule of the regions (outside the source or the output, an MCU of the output uncovered, more than
 * V1C_JPEG_XC_MAX_REGIONS of them), sizes, restart_mcus outside 0 ... 65535, capacity.  All before any device call.                    */
#define V1C_JPEG_XC_MAX_REGIONS 16
#define V1C_JPEG_XC_MAX_OUTPUTS 16
#define V1C_JPEG_HEADER_XC_MAX 2048           /* bytes v1c_jpeg_header_xc can write                                                 */

typedef struct v1c_jpeg_xc_region {   /* in MCUs                                                                                  */
    int32_t src_x, src_y, nx, ny, dst_x, dst_y;
} v1c_jpeg_xc_region;

typedef struct v1c_jpeg_xc_output {
    int32_t width, height;            /* pixels                                                                                  */
    int32_t restart_mcus;             /* MCUs per restart interval, 1 ... 65535; 0: no restart markers and no DRI                */
    int32_t optimize;                 /* != 0: Huffman tables of its own, as v1c_jpeg_encode_opt builds them                     */
    int32_t nregions, reserved;
    const v1c_jpeg_xc_region* regions;
    uint8_t* out_host;                /* HOST memory for the scan, page-locked recommended                                       */
    uint64_t capacity;                /* >= v1c_jpeg_transcode_bound of this output                                              */
    uint64_t size;                    /* out: bytes of its scan                                                                  */
    uint32_t dht_size;                /* out: bytes of dht, 0 for optimize == 0                                                  */
    uint8_t dht[V1C_JPEG_DHT_MAX];    /* out: the DHT segment's body                                                             */
} v1c_jpeg_xc_output;

/* Bytes the scan of a width x height output of the file can need (v1c_jpeg_bound's rule for the file's components and sampling).
 * Host-only.  0 for a file the transcoder refuses or sizes out of range.                                                          */
uint64_t v1c_jpeg_transcode_bound(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus);

/* Every check of v1c_jpeg_transcode that needs no device, and nothing else: the parse, the file's scope, every output's rules
 * (out_host and capacity are not looked at).  Touches no device.  *error_pos (may be NULL): where a parse stopped.               */
int v1c_jpeg_transcode_check(const uint8_t* file, uint64_t size, int n, const v1c_jpeg_xc_output* outputs, uint64_t* error_pos);

/* Everything of an output's file in front of its scan into the HOST buffer `out`: SOI, APP0 (JFIF), DQT with the FILE's tables, SOF0
 * (SOF1 where a table has 16-bit entries) with the output's size and the file's sampling factors, DHT (dht of dht_size bytes as
 * v1c_jpeg_transcode returned it, or NULL for the Annex K tables), DRI unless restart_mcus is 0, SOS.  The source's APPn and COM
 * segments are not carried over.  The output's file is these bytes, its scan and EOI.  Host-only.  Returns the number of bytes, or
 * the parse's code, or V1C_E_INVALID.                                                                                              */
int64_t v1c_jpeg_header_xc(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus, const uint8_t* dht,
                           uint32_t dht_size, uint8_t* out, uint64_t capacity);

/* Transcodes the file (HOST memory) into n outputs on `stream`: every out_host receives the scan of its output, `size` its size and,
 * for an optimising output, dht / dht_size its tables.  The scan is byte for byte what the encoder writes for the gathered
 * coefficients with those tables and that restart interval.  subseq_bits and report as v1c_jpeg_decode.  The call SYNCHRONISES the
 * stream once per round of the decode, once for the verdict on the stream and on the coefficients' range, and twice for the sizes
 * and the scans, as v1c_jpeg_encode_batch does.  V1C_E_UNSUPPORTED, before anything is done on the device, while `stream` is being
 * captured into a graph; V1C_E_CORRUPT where the last pass of the decode finds the entropy-coded data damaged (report->error_pos: the
 * bit); V1C_E_UNSUPPORTED where a coefficient of a GATHERED block is outside what 8-bit samples give (an AC coefficient beyond
 * +-1023, a DC outside -1024 ... 1023, judged before it is cut to 16 bits): the encoder's tables do not code it.  After an error the outputs' content is unspecified.                       */
int v1c_jpeg_transcode(int device, void* stream, const uint8_t* file, uint64_t size, int n, v1c_jpeg_xc_output* outputs,
                       uint32_t subseq_bits, v1c_jpeg_decode_report* report);

/* ---- lossless JPEG join, rotate and flip (INTEGRATION.md section 10 states the contract; tests/jpgxf_ref.py restates it) -------------
 * v1c_jpeg_transcode with up to V1C_JPEG_XF_MAX_SOURCES files and a transform per region.  A region is nx x ny MCUs of file `source`
 * from MCU (src_x, src_y), transformed and placed with the first MCU of the RESULT at MCU (dst_x, dst_y) of the output.  A transform is
 * three bits -- 4: transpose first, 1: then mirror x, 2: then mirror y --, so 0 none, 1 flip_h, 2 flip_v, 3 rot180, 4 transpose, 5
 * rot90 (clockwise), 6 rot270, 7 transverse.  MCUs move within the region, luma blocks within the MCU, coefficients within the block,
 * and coefficients of odd frequency along a mirrored axis change sign; no magnitude changes.  A region is placed as NX x NY MCUs:
 * nx x ny, or ny x nx where it transposes.  A transform acts on whole MCUs: what a partial last MCU column or row holds beyond the
 * image's edge moves with it.
 * Every source must be a file v1c_jpeg_transcode takes (its codes otherwise).  V1C_E_UNSUPPORTED for sources of different component
 * counts or sampling factors; for a transposing code on a file with h_samp != v_samp (4:2:2: the result would be 4:4:0); for regions
 * of an output whose effective quantisation tables -- the source's, transposed where the region transposes -- are not region 0's; and
 * for regions that overlap in an output.  V1C_E_INVALID for every other rule of the regions -- a source or transform out of range,
 * outside the source, the placed rectangle outside the output, an MCU of the output uncovered, more than
 * V1C_JPEG_XC_MAX_REGIONS of them --, for sizes, restart_mcus, capacity, and for nsources or n out of range.  All before any device
 * call.                                                                                                                           */
#define V1C_JPEG_XF_MAX_SOURCES 4

typedef struct v1c_jpeg_xf_source {
    const uint8_t* file;              /* HOST memory                                                                             */
    uint64_t size;
} v1c_jpeg_xf_source;

typedef struct v1c_jpeg_xf_region {   /* in MCUs                                                                                  */
    int32_t source, transform, src_x, src_y, nx, ny, dst_x, dst_y;
} v1c_jpeg_xf_region;

typedef struct v1c_jpeg_xf_output {   /* v1c_jpeg_xc_output with v1c_jpeg_xf_region regions                                       */
    int32_t width, height;
    int32_t restart_mcus;
    int32_t optimize;
    int32_t nregions, reserved;
    const v1c_jpeg_xf_region* regions;
    uint8_t* out_host;
    uint64_t capacity;                /* >= v1c_jpeg_compose_bound of this output                                                */
    uint64_t size;
    uint32_t dht_size;
    uint8_t dht[V1C_JPEG_DHT_MAX];
} v1c_jpeg_xf_output;

/* v1c_jpeg_transcode_bound for an output of files like `file` (any of the sources: the bound depends on the components and the
 * sampling factors alone).  Host-only.                                                                                            */
uint64_t v1c_jpeg_compose_bound(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus);

/* Every check of v1c_jpeg_compose that needs no device, and nothing else.  Touches no device.  error_pos (may be NULL): nsources
 * entries, where each source's parse stopped.                                                                                     */
int v1c_jpeg_compose_check(int nsources, const v1c_jpeg_xf_source* sources, int n, const v1c_jpeg_xf_output* outputs, uint64_t* error_pos);

/* v1c_jpeg_header_xc with the file's quantisation tables transposed where `transposed` is not 0: the header of an output whose
 * region 0 is of this file and transposes or not.  Host-only.                                                                     */
int64_t v1c_jpeg_header_xf(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus, int transposed, const uint8_t* dht,
                           uint32_t dht_size, uint8_t* out, uint64_t capacity);

/* Composes n outputs from nsources files (HOST memory) on `stream`, as v1c_jpeg_transcode does from one.  Each source is decoded in
 * turn up to its DC scan into a coefficient store of its own; the stream is SYNCHRONISED once per round of each decode, once per
 * call for the verdicts -- every source's entropy-coded data and the range of the gathered coefficients --, and twice for the sizes
 * and the scans.  reports (may be NULL): nsources entries, one per source; after V1C_E_CORRUPT from the device the damaged source's
 * error_pos is the bit, the others' 0.  V1C_E_UNSUPPORTED, before anything is done on the device, while `stream` is being
 * captured.                                                                                                                       */
int v1c_jpeg_compose(int device, void* stream, int nsources, const v1c_jpeg_xf_source* sources, int n, v1c_jpeg_xf_output* outputs,
                     uint32_t subseq_bits, v1c_jpeg_decode_report* reports);

/* ---- lateral chromatic aberration: one map per colour channel of a BGR remap ---------------------------------------------------
 * A lens magnifies red, green and blue by slightly different amounts; the correction is a radial rescaling of the source position
 * per channel, i.e. three chains that differ in radial stages in front of Denormalize (chromatic.py: transformer *
 * PolynomialScaler(coefs_c)).  A v1c_ca_plan takes the three lowered chains -- B, G, R, each as v1c_plan_create takes its one -- and
 * remaps uint8 BGR units so that byte c of every output pixel is what a v1c_plan of chain c writes there (same sizes, interpolation,
 * border mode and colour; under BORDER_TRANSPARENT a channel whose own footprint leaves the source keeps the destination's byte).
 * The numerical contract above carries over.  When the chains agree in everything but the radial composite behind the rotation and
 * every radial table is usable, the plan is FUSED: one ray direction per pixel, one table per distinct composite
 * (v1c_ca_plan_path 1); otherwise three fp64 interpreters run per pixel (path 0).
 *
 * v1c_ca_plan_run: launch-only (no allocation, no synchronisation), graph-capturable; 16 units per launch, longer arrays in several
 * launches; argument errors are reported before any device call; one plan may be run from several threads / streams (the ray pass,
 * its tile-flag words and the fix-up pass keep stream order through an event).  Units may override the rotation as for v1c_plan_run
 * when every chain has the same number (> 0) of rotate stages.
 * v1c_ca_plan_get_map: the float32 map of one channel (0 B, 1 G, 2 R), as v1c_plan_get_map.
 * v1c_ca_plan_last_launch: V1C_LAUNCH_CHROMA, | V1C_LAUNCH_FIXUP when a fix-up pass followed; -1 before the first run.            */
typedef struct v1c_ca_plan v1c_ca_plan;
int v1c_ca_plan_create(v1c_ca_plan** out, int device, const v1c_chain chains[3] /* B, G, R */, int src_h, int src_w, int dst_h,
                       int dst_w, int interp, int border_mode, const uint8_t border_val[4]);
int v1c_ca_plan_run(v1c_ca_plan* plan, void* stream, const v1c_unit* units, int n_units);
int v1c_ca_plan_get_map(v1c_ca_plan* plan, void* stream, int channel, float* xmap, float* ymap, int64_t map_pitch,
                        const double* rot_or_null);
int v1c_ca_plan_path(const v1c_ca_plan* plan);        /* 0 literal, 1 fused ray */
int v1c_ca_plan_last_launch(const v1c_ca_plan* plan);
int v1c_ca_plan_destroy(v1c_ca_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* VR180_REMAP_H */
