/*
 * tmat.h -- C-ABI of libtmat_hip.so: the MI355X (gfx950) implementation of the 2-D
 * microvessel-branching hot path of fogg-lab/tissue-model-analysis-tools
 * (scripts/compute_branches.py:307-361,391-426 and the fl_tissue_model_tools functions it drives).
 *
 * The reference is pure Python; a maintainer binds this library with ctypes (INTEGRATION.md shows
 * the stub).  All buffers are caller-owned, contiguous, row-major.  Every function returns 0 on
 * success or a negative code; tmat_last_error() returns a message for the calling thread.
 * No torch / Python types cross this boundary.  Functions taking a `tmat_handle` run on that
 * handle's HIP device and stream; a handle is not thread-safe, separate handles are independent.
 *
 * Pointer suffix convention:  *_dev arguments are HIP device pointers on the handle's device,
 * everything else is host memory.
 */
#ifndef TMAT_H
#define TMAT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tmat_ctx *tmat_handle;

#define TMAT_OK 0
#define TMAT_E_ARG (-1)     /* bad argument / unsupported shape            */
#define TMAT_E_HIP (-2)     /* HIP runtime error (message has the detail)  */
#define TMAT_E_WEIGHTS (-3) /* malformed weight blob                       */
#define TMAT_E_CAP (-4)     /* caller-provided output capacity too small   */

const char *tmat_last_error(void);
/* 0x00MMmmpp */
int tmat_version(void);

/*
 * Model life-cycle.  Replaces models.get_unet_patch_segmentor_from_cfg /
 * UNetXceptionPatchSegmentor.__init__ (reference models.py:600-622, 656-684): builds the
 * UNet-Xception of models.py:85-171 and loads its weights once per run (compute_branches.py:576).
 * `weights_blob` is the "TMATW001" container (tmat_amd/synth.py:pack_weights; Keras tensor
 * layouts) -- the offline stand-in for checkpoint_1.h5.
 * `max_patches` sizes the activation workspace, i.e. the UNet batch held in HBM at once (39 MB per patch; 0 = default
 * 400 = two 1024^2 images per pass).  It is not a limit on the image size: an image that needs more patches runs its
 * patch list in chunks, one image per pass.
 */
int tmat_create(int device_id, const void *weights_blob, size_t n_bytes, int max_patches, tmat_handle *out);
/* A handle without weights (device + stream only) for the entry points that need no model: tmat_zproj_*,
 * tmat_filter_edt_batch, tmat_finish_batch.  Model entry points return TMAT_E_ARG on it. */
int tmat_create_plain(int device_id, tmat_handle *out);
void tmat_destroy(tmat_handle h);
/* blocks until all work queued on the handle's stream is done */
int tmat_sync(tmat_handle h);

/* Bit depth of the images the next segment / analyze calls receive (16, the default, or 8).  Images always cross the
 * ABI as uint16; cv2.resize saturates its result to the depth of its input (compute_branches.py:309-312), so 8-bit
 * sources (widened by the caller) must saturate the Lanczos overshoot at 255 instead of 65535. */
int tmat_set_input_depth(tmat_handle h, int bits);

/*
 * keras_model.predict on a patch batch (reference models.py:644 as called from
 * smooth_tiled_predictions.py:179,182): x (n, P, P) f32 -> y (n, P, P) f32 sigmoid output
 * (the trailing channel axis of size 1 is implicit).  P = patch size of the blob (320).
 */
int tmat_unet_predict(tmat_handle h, const float *x, int n, float *y);

/*
 * UNetXceptionPatchSegmentor.predict(x, auto_resample=False) (reference models.py:624-653) =
 * predict_img_with_smooth_windowing(x, window_size=P, subdivisions=2, pred_func=model.predict)
 * (smooth_tiled_predictions.py:220-267): pad, 8 D4 copies, 50 %-overlap tiles, UNet, squared-spline
 * window, f64 overlap-add, D4 undo + mean, unpad.  x: (n, h, w) f32; pred: (n, h, w) f64.
 */
int tmat_predict_smooth(tmat_handle h, const float *x, int n, int hh, int ww, double *pred);

/*
 * The same for any `subdivisions` (smooth_tiled_predictions.py:220-267 with the library's own network as pred_func; the reference's
 * comments :242-247 name 4).  subdivisions == 2 IS tmat_predict_smooth: the same code path, launches and region forms.  Any other
 * value applies the input norm (tmat_set_input_norm) likewise, tiles with the general geometry of tmat_smooth_plan, runs the network
 * full-frame in chunks of at most max_patches and blends on the device; the tile predictions (n_tiles P P floats) are allocated for
 * the call, TMAT_E_HIP when that fails.
 */
int tmat_predict_smooth_ex(tmat_handle h, const float *x, int n, int hh, int ww, int subdivisions, double *pred);

/*
 * Smooth tiling around a predictor the CALLER runs (a Keras model.predict, say): the stage between tmat_preprocess_batch and
 * tmat_postprocess_batch for a lab that keeps its own network.  Replaces everything of predict_img_with_smooth_windowing
 * (smooth_tiled_predictions.py:220-267) but the pred_func calls of :174-182, for a 2-D single-channel image, any window_size >= 4
 * and any 2 <= subdivisions <= window_size, bit for bit.
 *
 * tmat_smooth_plan (host, no handle) -- the geometry of _pad_img :74, _windowed_subdivs :152-163:
 *   aug = int(round(ws (1 - 1 / s))) (Python's round: 4.5 -> 4, 7.5 -> 8), step = int(ws / s); the padded image is
 *   (hh + 2 aug) x (ww + 2 aug); eight frames in the order of _rotate_mirror_do :95-113, even ones padded-height x padded-width, odd
 *   ones transposed; per frame na x nb tiles at i, j in range(0, side - ws + 1, step), row-major.  counts = {na, nb of the even
 *   frames, na, nb of the odd ones}; n_tiles their sum over the eight frames.  Global tile index: frame, then a, then b.  The step need
 *   not divide side - ws: the strip no tile covers contributes 0.0 in that frame, as in the reference.  Any output pointer may be
 *   null.  TMAT_E_ARG for window_size < 4, subdivisions < 2 or > window_size, an empty image, a frame side below window_size (the
 *   reference returns an empty array or crashes on these).
 * tmat_spline_window (host, no handle) -- _spline_window :26-41: win[window_size] f64, window_size >= 4, odd sizes included.
 *
 * The session, on any handle (tmat_create_plain is enough); one per handle, a second begin discards an open one:
 * tmat_smooth_begin   uploads x (hh, ww) f32 and takes its minimum, the pad value of :77.  tmat_set_input_norm does not apply: the
 *                     caller owns x.
 * tmat_smooth_tiles   patches (count, ws, ws) f32 = the tiles [first, first + count), what :157-171 builds; any ranges, any order.
 * tmat_smooth_put     preds (count, ws, ws) of dtype TMAT_SMOOTH_F32 or TMAT_SMOOTH_F64 = pred_func's results for those tiles (the
 *                     trailing channel axis of size 1 implicit).  A session holds one dtype: a float64 put into a float32 session
 *                     widens what is stored (no bit of the result changes), a float32 put into a float64 session is TMAT_E_ARG.  The
 *                     buffer, n_tiles ws ws values (968 tiles, 400 MB at 640 x 640, ws 320, subdivisions 4), is allocated by the
 *                     first put: TMAT_E_HIP when that fails.
 * tmat_smooth_end     out (hh, ww) f64 = :185-265 (window, overlap-add, / s^2, D4 undo, mean, unpad); releases the session.
 *                     TMAT_E_ARG, with the session left open, while a tile has not been put.
 * A tile range outside [0, n_tiles) and a call without an open session are TMAT_E_ARG.
 */
#define TMAT_SMOOTH_F32 0
#define TMAT_SMOOTH_F64 1
int tmat_smooth_plan(int hh, int ww, int window_size, int subdivisions, int *aug, int *step, int counts[4], int *n_tiles);
int tmat_spline_window(int window_size, double *win);
int tmat_smooth_begin(tmat_handle h, const float *x, int hh, int ww, int window_size, int subdivisions, int *n_tiles);
int tmat_smooth_tiles(tmat_handle h, int first, int count, float *patches);
int tmat_smooth_put(tmat_handle h, int first, int count, const void *preds, int dtype);
int tmat_smooth_end(tmat_handle h, double *out);
/*
 * PIL.Image.fromarray(x float32).resize((out_w, out_h), resample) for n mode-"F" images (n, H, W) -> (n, out_h, out_w): the two
 * calls UNetXceptionPatchSegmentor.predict(x, auto_resample=True) makes around the smooth prediction (reference models.py:631-635
 * LANCZOS, :647-651 NEAREST).  filter: TMAT_PIL_NEAREST or TMAT_PIL_LANCZOS (Pillow's own numbers).  Bit for bit Pillow's result
 * (checked against Pillow 12.2.0): the convolution resample with f64 taps and f64 sums stored as f32, horizontal pass first, a pass
 * whose sizes are equal skipped; the affine nearest scale whose source coordinate accumulates.  Sizes up to 32768 a side.
 * tmat_resize_pil_f32 runs on the handle's device (tmat_create_plain is enough; the tap tables are made on the host and uploaded),
 * tmat_host_resize_pil_f32 is its host twin.
 *
 * tmat_predict_auto_resample -- predict(x, auto_resample=True) (models.py:624-653) for one image without leaving the device: upload x
 * (H, W) -> LANCZOS to (mid_h, mid_w) -> the input norm where tmat_set_input_norm is on (:637-638) -> the smooth prediction of
 * tmat_predict_smooth -> float32 (Image.fromarray of a float64 array makes a mode-"F" image) -> NEAREST to (out_h, out_w) -> download.
 * The reference hands Pillow its (rows, cols) shapes as sizes, which Pillow reads as (width, height): for an H x W input and
 * target_shape = round((H, W) ds_ratio) = (th, tw) the caller passes mid = (tw, th) and out = (W, H), as the Python mirror does.
 */
#define TMAT_PIL_NEAREST 0
#define TMAT_PIL_LANCZOS 1
int tmat_resize_pil_f32(tmat_handle h, const float *x, int n, int H, int W, int out_h, int out_w, int filter, float *out);
int tmat_host_resize_pil_f32(const float *x, int n, int H, int W, int out_h, int out_w, int filter, float *out);
int tmat_predict_auto_resample(tmat_handle h, const float *x, int H, int W, int mid_h, int mid_w, int out_h, int out_w, float *out);

/* Measurement only (tools/bench_smooth.py): device time, by HIP events, of the tile-gather launches and of the blend launch of the
 * handle's last session. */
int tmat_debug_smooth_times(tmat_handle h, double *tiles_ms, double *blend_ms);

/*
 * compute_branches.py:309-328 for a batch: cv2.resize(img, round(shape * ds_ratio), INTER_LANCZOS4)
 * -> rescale_intensity(out_range=(0,1)).astype(f32) -> model.predict(auto_resample=False).
 * imgs: (n, H, W) u16; pred: (n, round(W*ds_ratio), round(H*ds_ratio)) f64 -- the reference passes its target shape to
 * cv2.resize as dsize, which cv2 reads as (width, height), so rows and columns swap roles for non-square images
 * (the later resize to the 384-wide field restores the aspect ratio); square images are unaffected.
 */
int tmat_segment_batch(tmat_handle h, const uint16_t *imgs, int n, int H, int W, double ds_ratio, double *pred);

/*
 * compute_branches.py:334-361 for a batch: pred > 0.5 -> filter_branch_seg_mask
 * (transforms.py:306-361) -> medial_axis + EDT centre-line weighting -> skimage resize to
 * img_dsamp_res = (out_h, out_w) (compute_branches.py:218-222: round(orig_shape * 384 / orig_width)),
 * order 1, anti-aliased -> f32.   pred: (n, h, w) f64; field: (n, out_h, out_w) f32.
 * Runs on the handle's device like the batch pipeline: threshold, filter, EDT, ordered medial-axis thinning (only its
 * tie-break permutation is made on the host), EDT of the skeleton, weighting, resize.
 * A handle from tmat_create_plain is enough.
 */
int tmat_postprocess_batch(tmat_handle h, const double *pred, int n, int hh, int ww, int out_h, int out_w, float *field);

/*
 * The GPU part of the above (csrc/morph_kernels.hip): pred > 0.5 -> filter_branch_seg_mask
 * (transforms.py:306-361, remove_isolated=True) -> EDT of the filtered mask (the `distance` output of
 * medial_axis(seg_mask, return_distance=True), compute_branches.py:340).
 * pred (n, h, w) f64; filtered (n, h, w) u8; dist (n, h, w) f64.  Needs a handle (runs on its device).
 */
int tmat_filter_edt_batch(tmat_handle h, const double *pred, int n, int hh, int ww, uint8_t *filtered, double *dist);

/*
 * The two pixel stages in front of the UNet on their own (compute_branches.py:309-316): cv2.resize(img, round(shape *
 * ds_ratio), INTER_LANCZOS4) and rescale_intensity(out_range=(0, 1)).astype(float32), on the device.  imgs (n, H, W) u16
 * host; x (n, round(W ds_ratio), round(H ds_ratio)) f32 host.  This is the image `make_well_mask` sees when --detect-well
 * is given (:318-319); tmat_predict_smooth continues from it.
 */
int tmat_preprocess_batch(tmat_handle h, const uint16_t *imgs, int n, int H, int W, double ds_ratio, float *x);

/*
 * Well detection (--detect-well), device stages of fl_tissue_model_tools/well_mask_generation.py:
 *   tmat_well_threshold = auto_threshold_well (:236-277): skimage gaussian(sigma 1) -> rescale_intensity(0..255) -> uint8 ->
 *     corner medians decide whether to invert -> skimage.filters.threshold_otsu (256-bin histogram kernel + a decision
 *     kernel that evaluates the inter-class variance exactly as numpy does) -> binary_erosion(footprint=disk(5)).
 *     img (H, W) f32 host -> out (H, W) u8 host.  H, W >= 20.
 *   tmat_canny_mask = skimage.feature.canny(mask, sigma) of a boolean image, default thresholds (:165, :201): mask, edges
 *     (H, W) u8 host.
 * The small host steps between them (nearest-neighbour rescale to <= 200 px, scipy.spatial.ConvexHull, the hull mask, the
 * seeded random superellipse search :16-91) are Python host code in tmat_amd/well_mask_generation.py.
 * A handle from tmat_create_plain is enough.
 */
int tmat_well_threshold(tmat_handle h, const float *img, int H, int W, uint8_t *out);
/* the same for a float64 image: integer images (compute_cell_area.py:127) enter skimage's gaussian through img_as_float */
int tmat_well_threshold_f64(tmat_handle h, const double *img, int H, int W, uint8_t *out);
int tmat_canny_mask(tmat_handle h, const uint8_t *mask, int H, int W, double sigma, uint8_t *edges);
/* n masks of one shape (n, H, W) in one launch set; every mask comes out as from tmat_canny_mask alone (padding, borders and the
 * hysteresis labels are per image).  n H W <= 2^26. */
int tmat_canny_mask_batch(tmat_handle h, const uint8_t *masks, int n, int H, int W, double sigma, uint8_t *edges);
/* The shape generate_well_mask searches on (:153-155): round((h, w) * min(1, 200 / max(h, w))), half to even.  Host only. */
int tmat_well_small_shape(int h, int w, int *small_h, int *small_w);
/*
 * Front end of --detect-well for n Z stacks of one shape that are resident in device memory (compute_branches.py:227-238 and
 * generate_well_mask up to the ConvexHull call, :153-170), one launch set for all n.  Per stack: max projection; anti-aliased
 * resize to (out_h, out_w) float64 (the arithmetic of tmat_resize_aa_u16 on that one image, its own clip range);
 * auto_threshold_well; nearest resize to the small shape (sh, sw) of tmat_well_small_shape(out_h, out_w); canny(sigma 1) of the
 * small mask plus the mask's own pixels on the image border.  Extrema, histograms, corner medians, the Otsu decision and the
 * borders of erosion and canny are per stack: a stack leaves a batch exactly as tmat_well_threshold_f64 + tmat_canny_mask
 * give it alone.
 * stacks_dev (n, Z, H, W) u16 device (tmat_dev_alloc), read only.  Host outputs: proj_aa_out NULL or (n, out_h, out_w) f64;
 * thresh_small, border_small (n, sh, sw) u8.  out_h, out_w >= 20, n out_h out_w <= 2^26.  The gaussian tables are those of
 * tmat_resize_aa_u16 and tmat_well_threshold.  A handle from tmat_create_plain is enough; scratch comes from the handle's pool.
 */
int tmat_stack_well_front_dev(tmat_handle h, const uint16_t *stacks_dev, int n, int Z, int H, int W, int out_h, int out_w,
                              double *proj_aa_out, uint8_t *thresh_small, uint8_t *border_small);
/*
 * The same front end for the cell-area tool (compute_cell_area.py:127 hands generate_well_mask the down-sampled INTEGER image;
 * well_mask_generation.py:153-170): small_dev (n, hh, ww) u16 device (tmat_cell_small_dev), read only.  Per image: img_as_float,
 * (double)v * (1.0 / 65535.0), or 1.0 / 255.0 for src_bits == 8 (explicit; the handle's input depth is not read);
 * auto_threshold_well; nearest resize to the small shape (sh, sw) of tmat_well_small_shape(hh, ww); canny(sigma 1) plus the mask's
 * own pixels on the image border.  An image leaves a batch exactly as tmat_well_threshold_f64 + tmat_canny_mask give it alone.
 * Host outputs: thresh_small, border_small (n, sh, sw) u8.  n >= 1, hh, ww >= 20, small shape >= 3 x 3, n hh ww <= 2^26, src_bits 8
 * or 16: TMAT_E_ARG otherwise, nothing written.  The gaussian table is that of tmat_well_threshold; scratch comes from the handle's pool.
 */
int tmat_cell_well_front_dev(tmat_handle h, const uint16_t *small_dev, int n, int hh, int ww, int src_bits, uint8_t *thresh_small,
                             uint8_t *border_small);

/*
 * The superellipse fit of well detection on the device (csrc/wellfit_kernels.hip), for a batch of images.
 *
 * tmat_superellipse_table: the candidates of get_superellipse_hull (well_mask_generation.py:35-45) depend on (seed, num_iters) alone.
 *   The host draws them once and uploads table (num_iters, 7) f64 = c_x, c_y, cos t, sin t, d s_a, d s_b, area per candidate, area by
 *   the reference's expression (:79-82: 4 d^2 s_a s_b gamma(1 + 1/n)^2 / gamma(1 + 2/n), so it belongs to ONE exponent n: a caller with
 *   images of several exponents uploads and searches once per exponent).  The table stays on the handle; the device evaluates no cos,
 *   sin or gamma.
 * tmat_superellipse_search replaces :47-91.  xy: the (x, y) f64 hull points of all images, concatenated; offs (n_imgs + 1): image i owns
 *   the points offs[i] .. offs[i + 1] - 1, 1 to 1024 of them (more: TMAT_E_CAP); n_exp (n_imgs): the exponent per image, 1..64 (else
 *   TMAT_E_ARG).  best[i]: index of the smallest-area candidate whose maximum over the image's points is certainly below 1, -1 when
 *   there is none; equal areas resolve to the lowest index, as np.argmin does.  n == 2 (the reference squares, without rotation) is
 *   bit-identical to numpy and decides every candidate.  For n != 2 the reference calls pow and the device multiplies n - 1 times (at
 *   most (n - 1) 2^-53 relative per term), so a candidate is decided only when |max - 1| > 1e-12; the others come back in band_idx
 *   (cap_band, 2) i32 as (image, candidate) pairs in ascending order, *n_band of them (more than cap_band: TMAT_E_CAP with *n_band set),
 *   for the caller to evaluate with the reference's expression and to merge with best by (area, index).
 * tmat_superellipse_masks replaces gen_superellipse_mask (:94-118) for n_masks masks of one shape.  params (n_masks, 6) f64 = c_x, c_y,
 *   cos t, sin t, d s_a, d s_b; xs (H), ys (W): np.linspace(-1, 1, .) made by the host; out (n_masks, H, W) u8:
 *   out[m, i, j] = |u|^n + |v|^n < 1 at x = xs[i], y = ys[j] (the orientation after the reference's swapaxes).  The same band rule per
 *   pixel for n != 2: band_px (cap_band) i64 flat indices into out, ascending, which the caller patches.
 * tmat_resize_nearest_u8: skimage resize(order=0) of n u8 images (n, H, W) -> (n, out_h, out_w), source index
 *   floor((i + 0.5) n_in / n_out) in f64 (:209 takes the small-shape well mask to the image shape with it).
 * Host buffers throughout.  A handle from tmat_create_plain is enough.
 */
int tmat_superellipse_table(tmat_handle h, const double *table, int num_iters);
int tmat_superellipse_search(tmat_handle h, const double *xy, const int *offs, int n_imgs, const int *n_exp, int *best, int *band_idx,
                             int cap_band, int *n_band);
int tmat_superellipse_masks(tmat_handle h, const double *params, int n_masks, const int *n_exp, const double *xs, const double *ys, int H, int W,
                            uint8_t *out, long long *band_px, int cap_band, int *n_band);
int tmat_resize_nearest_u8(tmat_handle h, const uint8_t *in, int n, int H, int W, int out_h, int out_w, uint8_t *out);

/*
 * transforms.filter_branch_seg_mask(mask, footprint, remove_isolated) (transforms.py:306-361) on the GPU for a batch of
 * uint8 masks: use_median 1 = footprint disk(2) (the default), 0 = footprint None (compute_branches.py:293).
 * mask, filtered (n, h, w) u8.  A handle from tmat_create_plain is enough.
 */
int tmat_filter_mask_batch(tmat_handle h, const uint8_t *mask, int n, int hh, int ww, int use_median, int remove_isolated,
                           uint8_t *filtered);

/*
 * skimage.morphology.medial_axis(mask, return_distance=True) (reference call compute_branches.py:340; scikit-image
 * 0.18.3 semantics with the RandomState(0) tie-break) for a batch, on the device: exact EDT (morph_kernels.hip), then the
 * ordered thinning (thin_kernels.hip: keys from distance / corner score / tie-break; a pixel's decision depends only on
 * its 8 neighbours with smaller keys, so the removal order is resolved as a dependency wavefront in strict Jacobi rounds).
 * Only the tie-break permutation (a Mersenne-Twister shuffle that depends on the foreground COUNT alone) is produced on
 * the host.  mask, skel (n, h, w) u8; dist (n, h, w) f64.  Images with h^2 + w^2 >= 2^27 are refused here (the squared
 * distance no longer fits its key field); the pipeline runs those through the host implementation
 * (tmat_host_medial_axis).  A handle from tmat_create_plain is enough.
 */
int tmat_medial_axis_batch(tmat_handle h, const uint8_t *mask, int n, int hh, int ww, uint8_t *skel, double *dist);

/*
 * The GPU stages after the medial-axis thinning (csrc/finish_kernels.hip): centerline_dt = EDT(~skel),
 * pred *= dist / (dist + centerline_dt) (compute_branches.py:341-344), skimage resize to (out_h, out_w)
 * (order 1, anti-aliased, :351-357) -> field f32, and rescale_intensity(field, (0, 255)) (:419) -> field255 f32.
 * pred, dist (n, h, w) f64; skel (n, h, w) u8; field, field255 (n, out_h, out_w) f32.
 */
int tmat_finish_batch(tmat_handle h, const double *pred, const double *dist, const uint8_t *skel, int n, int hh, int ww,
                      int out_h, int out_w, float *field, float *field255);

/*
 * fl_tissue_model_tools.dmtgraph.compute_dmt_graph(img, delta1, delta2) (reference
 * dmtgraph.py:38-99; the contract the un-vendored pydmtgraph C++ extension exposed).
 * img: (rows, cols) f32.  verts: (cap_v, 2) int32 [row, col]; edges: (cap_e, 2) int32.
 * With a handle the edge keys, the lower-star sort and both persistence sweeps run on its device
 * (TMAT_DMT_SWEEP_DEVICE=0: the sweeps on the host), `collect` on the host; `h` may be NULL
 * (host-only execution, sequential sweeps).
 */
int tmat_dmt_graph(tmat_handle h, const float *img, int rows, int cols, float delta1, float delta2,
                   int32_t *verts, int cap_v, int32_t *edges, int cap_e, int *n_verts, int *n_edges);

/*
 * The same for n fields of one shape in one call -- the loop over images around compute_dmt_graph
 * (reference topology.py:148-160 per image, scripts/compute_branches.py:585-594 over images): edge keys,
 * the lower-star sort and the two persistence sweeps of all fields run as one launch each
 * (dmtgraph.py:57-93, :277-314), `collect` (dmtgraph.py:317-453) per field on host threads.
 * imgs: (n, rows, cols) f32.  verts: (n, cap_v, 2) int32, edges: (n, cap_e, 2) int32; n_verts, n_edges: (n).
 */
int tmat_dmt_graph_batch(tmat_handle h, const float *imgs, int n, int rows, int cols, float delta1, float delta2,
                         int32_t *verts, int cap_v, int32_t *edges, int cap_e, int *n_verts, int *n_edges);

/*
 * topology.MorseGraph(img, thresholds, min_branch_length, max_branch_length,
 * remove_isolated_branches, smoothing_window, pruning_mask) downstream of compute_dmt_graph
 * (reference topology.py:148-179, 181-356): smoothing, trimming, spanning forest, branch labels,
 * barcode, min-length filter.  verts/edges are compute_dmt_graph's outputs.
 * max_branch_length <= 0 means None.  pruning_mask (rows, cols) u8 or NULL.
 * Outputs: *count = len(barcode); *total_px = get_total_branch_length();
 * *avg_px = get_average_branch_length(); bars (cap, 2) f64 [birth, death] (may be NULL).
 */
int tmat_morse_stats(const int32_t *verts, int n_verts, const int32_t *edges, int n_edges, int rows, int cols,
                     int smoothing_window, int min_branch_length, int max_branch_length,
                     int remove_isolated_branches, const uint8_t *pruning_mask, int64_t *count,
                     double *total_px, double *avg_px, double *bars, int cap);

/*
 * The branch geometry MorseGraph.__compute_colored_tree_and_barcode(scaling_factor) builds (reference topology.py:358-389)
 * for the branches that survive __filter_graph (:318-347), in the reference's order.  Same inputs and the same graph code
 * as tmat_morse_stats, plus scaling_factor; needs no handle and no GPU.
 * Per branch, _vertices[branch_vertices] * scaling_factor (float32, :380) goes through __moving_average_fixed_ends(., 3)
 * (:458-515; branches of one or two vertices are returned unchanged, :470-471) and every pair of neighbours becomes one
 * segment with the coordinates reversed (:386): x = column, y = row.
 * segs (cap_s, 4) f64 [x1, y1, x2, y2]; seg_branch (cap_s) i32: index of the segment's branch; bars (cap_b, 2) f64
 * [birth, death] * scaling_factor (:377), branch order; *n_segs, *n_bars: what was (or would be) written.
 * *count, *total_px, *avg_px: as tmat_morse_stats returns them (unscaled).  TMAT_E_CAP when cap_s or cap_b is too small
 * (*n_segs and *n_bars then hold the sizes needed).
 */
int tmat_morse_tree(const int32_t *verts, int n_verts, const int32_t *edges, int n_edges, int rows, int cols,
                    int smoothing_window, int min_branch_length, int max_branch_length,
                    int remove_isolated_branches, const uint8_t *pruning_mask, double scaling_factor, int64_t *count,
                    double *total_px, double *avg_px, double *segs, int32_t *seg_branch, int cap_s, double *bars,
                    int cap_b, int *n_segs, int *n_bars);

/*
 * Colour of branch i (reference topology.py:518-527, __random_color): hue byte = floor(180 * 0.618033988749895 * i) mod 256
 * (the uint8 wrap of the reference's pinned numpy), H = 2 * hue byte degrees mod 360, S = 220 / 255, V = 1, the standard
 * HSV -> RGB sextant formula in f64, each channel floor(255 v + 0.5).  The reference hands cv2's (B, G, R) triple to
 * matplotlib as (R, G, B); rgb[] keeps that swap: rgb = (B, G, R).  cv2's own 8-bit HSV rounding is not pinned.
 */
int tmat_branch_color(int i, uint8_t *rgb);

/*
 * The tree overlay of compute_branches.py:431-450 (morse_tree*.png) as an RGB8 raster of the project's own specification
 * (DESIGN.md "Tree overlay and barcode pictures"; matplotlib's pixels are not reproduced): the min-max rescaled background
 * (:447) sampled nearest onto a vis_width x round_half_even(vis_width bh / bw) canvas, every segment a capsule of
 * matplotlib's default 1.5 pt line width at 200 dpi, composited in segment order.  Batched: n backgrounds (n, bh, bw),
 * bg_dtype 0 = u16, 1 = f32; segs (seg_offsets[n], 4) f64 in background pixels and seg_branch as tmat_morse_tree returns
 * them, image i owning [seg_offsets[i], seg_offsets[i + 1]); rgb_out (n, vh, vw, 3) u8.  All pointers are host pointers.
 * f32 backgrounds must be finite (a NaN or infinity makes the minimum / maximum, and so the picture, undefined); segments with a
 * non-finite coordinate are skipped.
 * tmat_render_tree rasterises on the handle's device (overlay_kernels.hip); tmat_host_render_tree is its host twin:
 * the same bytes, no handle, no GPU.  tmat_render_tree_timed is tmat_render_tree that also reports where the call's time goes:
 * ms4 = HIP-event milliseconds on the call's stream of {upload, min-max kernels, render kernels, copy back of the overlays}
 * (tools/bench_overlay.py).
 */
int tmat_render_tree(tmat_handle h, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs,
                     const int32_t *seg_branch, const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out);
int tmat_render_tree_timed(tmat_handle h, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs,
                           const int32_t *seg_branch, const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out, float *ms4);
int tmat_host_render_tree(const void *background, int bg_dtype, int n, int bh, int bw, const double *segs,
                          const int32_t *seg_branch, const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out);

/*
 * plot_colored_barcode (reference topology.py:67-107) without axes or text: a white square canvas of
 * round_half_even(0.9 vis_width) pixels, the bars (n, 2) f64 of tmat_morse_tree sorted by birth, descending and stable, bar k
 * a rectangle of 0.8 row pitch on row k (row 0 lowest) from birth to death in the colour of its branch, the range
 * [min birth, max death] mapped onto the width; integer pixel edges, no anti-aliasing.  rgb_out (S, S, 3) u8.
 * tmat_host_render_barcode runs on the host.  tmat_render_barcode is the batched device form (overlay_kernels.hip): bars
 * (bar_offsets[n_pics], 2) f64 and bar_offsets (n_pics + 1) int32, host pointers, picture p owning the bars
 * [bar_offsets[p], bar_offsets[p + 1]); rgb_out (n_pics, S, S, 3) u8 host.  The host keeps the sort, the edge rounding and the colours
 * and hands the device a table of rectangles; the bytes are the host form's for every input (no bars, a zero span, more bars than
 * rows).  tmat_render_barcode_png returns the same canvases as PNG files (render and encoder back to back on the handle's stream, as
 * tmat_render_tree_png; its bound is tmat_png_bound(S, S, 3)).  A handle from tmat_create_plain is enough.
 * tmat_host_barcode_rects (tests): the rectangle table of one picture, five int32 each -- columns [xa, xb), rows [ya, yb) counted from
 * the bottom row, rgb = r | g << 8 | b << 16 --, entry k being row k of the sorted order; *n_rects is 0 when nothing is drawn.
 */
int tmat_host_render_barcode(const double *bars, int n, int vis_width, uint8_t *rgb_out);
int tmat_render_barcode(tmat_handle h, const double *bars, const int32_t *bar_offsets, int n_pics, int vis_width, uint8_t *rgb_out);
int tmat_render_barcode_png(tmat_handle h, const double *bars, const int32_t *bar_offsets, int n_pics, int vis_width, uint8_t *out,
                            size_t cap_each, size_t *sizes);
int tmat_host_barcode_rects(const double *bars, int n, int vis_width, int32_t *rects_out, int cap, int *n_rects);

/*
 * save_vis, the picture rule of the 2-D and Z-stack branches (compute_branches.py:74-78: rescale_intensity(out_range=(0, 255)) and
 * cv2.imwrite's cast; :315 original_image.png, :331 prediction.png, :347 segmentation_mask.png, :348 distance_transform.png, :228-229
 * and :303 the two pictures of a stack), for n images of `per` pixels.  Per image, in f64: lo / hi = minimum / maximum over the
 * non-NaN values; v = ((a - lo) / (hi - lo)) * 255 when hi != lo, min(max(a, 0), 255) otherwise; NaN becomes 0; out = (u8) rint(v),
 * ties to even.  An image that is all NaN gives an all-zero picture.  Infinities are outside the contract (the extrema, and so the
 * picture, are then undefined), as they are for tmat_render_tree.
 * a: (n, per) of dtype TMAT_PIC_*, out: (n, per) u8, both host pointers.  tmat_stage_pictures runs on the handle's device
 * (vis_kernels.hip; a handle from tmat_create_plain is enough); tmat_host_stage_pictures is its host twin: the same bytes, no GPU.
 */
#define TMAT_PIC_U16 0
#define TMAT_PIC_F32 1
#define TMAT_PIC_F64 2
#define TMAT_PIC_U8 3
int tmat_stage_pictures(tmat_handle h, const void *a, int dtype, int n, size_t per, uint8_t *out);
int tmat_host_stage_pictures(const void *a, int dtype, int n, size_t per, uint8_t *out);

/*
 * PNG files made on the device (csrc/png_kernels.hip), for the pictures above: n pictures of one shape (H, W) with
 * `channels` = 1 (grey, colour type 0) or 3 (RGB, colour type 2), u8, contiguous -> n complete files: signature, IHDR, IDAT chunks,
 * IEND; bit depth 8, no interlace, no ancillary chunk.  One filter type per row out of None / Sub / Up / Average / Paeth by the
 * minimum sum of absolute signed residuals (ties: the lowest type); the filtered stream cut into stripes of tmat_png_stripe bytes,
 * each compressed on its own (LZ77 inside the stripe, one fixed-Huffman or stored block, whichever is smaller) into its own IDAT
 * chunk, so that the chunks concatenate into one zlib stream.  The bytes of a file depend on the picture and (H, W, channels) only.
 * File i occupies out + i * cap_each for sizes[i] bytes; out and sizes are host pointers, bytes past sizes[i] are not written.
 * cap_each below the bound of tmat_png_bound: TMAT_E_CAP, nothing written.  H or W < 1, channels outside {1, 3}, or a filtered
 * stream H (W channels + 1) of 2^31 bytes or more: TMAT_E_ARG.  n == 0 succeeds.  A handle from tmat_create_plain is enough; device
 * memory comes from the handle's pool on first use.
 * tmat_png_encode_batch takes host pictures, tmat_png_encode_batch_dev device pictures, tmat_host_png_encode_batch is the host twin:
 * the same bytes, no handle, no GPU.  tmat_png_encode_batch_timed is tmat_png_encode_batch that also reports ms3 = HIP-event
 * milliseconds on the handle's stream of {upload, kernels, copy back of sizes and files} (tools/bench_png.py).
 * tmat_render_tree_png takes the arguments of tmat_render_tree and returns the overlays as PNG files: render and encoder run back to
 * back on the handle's stream and the raw (n, vh, vw, 3) overlays stay on the device; its bound is tmat_png_bound of (vh, vw, 3).
 */
int tmat_png_stripe(void);
int tmat_png_bound(int H, int W, int channels, size_t *bound);
int tmat_png_encode_batch(tmat_handle h, const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes);
int tmat_png_encode_batch_dev(tmat_handle h, const uint8_t *pics_dev, int n, int H, int W, int channels, uint8_t *out, size_t cap_each,
                              size_t *sizes);
int tmat_png_encode_batch_timed(tmat_handle h, const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each,
                                size_t *sizes, float *ms3);
int tmat_host_png_encode_batch(const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes);
int tmat_render_tree_png(tmat_handle h, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs,
                         const int32_t *seg_branch, const int32_t *seg_offsets, int vis_width, uint8_t *out, size_t cap_each, size_t *sizes);

/*
 * The encoder's two modes.  TMAT_PNG_FAST (the default) is the encoder described above.  TMAT_PNG_COMPACT (opt-in) keeps the filter,
 * the stripes, the match rule and tmat_png_bound and changes the parse and the blocks: a match gives way to a literal when the match at
 * the next position is longer (one-step lazy), and every stripe becomes a stored, a fixed-Huffman or a dynamic-Huffman block
 * (RFC 1951 3.2.7: code lengths from the stripe's own histograms, limited to 15 bits, header trimmed and run-length coded), whichever
 * is the fewest bytes by exact count, the earlier of the three on a tie.  A compact file is again a function of the picture and
 * (H, W, channels) alone, and the device and the host twin produce the same bytes.
 * tmat_png_set_mode: a property of the handle, like tmat_set_precision.  It applies to the calls that follow and covers every entry
 * point that encodes -- tmat_png_encode_batch, _dev and _timed, tmat_render_tree_png, tmat_render_barcode_png and the tree_png /
 * barcode_png outputs of tmat_analyze_batch_grid*.  A handle from tmat_create_plain is enough.  Any other mode: TMAT_E_ARG, the handle
 * keeps its mode.
 * tmat_host_png_encode_batch_mode: the host twin with the mode as an argument (tmat_host_png_encode_batch is its TMAT_PNG_FAST); a
 * mode outside the two: TMAT_E_ARG, nothing written.
 * tmat_host_png_code_lengths (test entry): the code lengths both implementations derive from a histogram freq[0, n): len[i] = 0
 * exactly where freq[i] = 0, no length above limit, Kraft sum exactly 1, and the optimal total cost wherever the Huffman tree is no
 * deeper than limit.  A histogram with ONE used symbol gets the one-bit code (Kraft sum 1/2: no complete set has one member; the
 * encoder never asks for it).  1 <= n <= 286, 1 <= limit <= 15, 2^limit >= n, sum of the frequencies below 2^22; else TMAT_E_ARG.
 * tmat_debug_png_code_lengths: the same function on the device for k histograms (freqs (k, n) u32, lens (k, n) u8, host pointers) in
 * one launch, one lane each; the same argument rules for every histogram; k == 0 succeeds.
 */
#define TMAT_PNG_FAST 0
#define TMAT_PNG_COMPACT 1
int tmat_png_set_mode(tmat_handle h, int mode);
int tmat_host_png_encode_batch_mode(const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes,
                                    int mode);
int tmat_host_png_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len);
int tmat_debug_png_code_lengths(tmat_handle h, const uint32_t *freqs, int k, int n, int limit, uint8_t *lens);

/*
 * TIFF pixels decoded on the device (csrc/tiff.h, tiff_host.cpp, tiff_kernels.hip): the ingest-side counterpart of the
 * PNG encoder.  It replaces the per-page host decode of the reference's helper.py:23-95 (load_image: PIL's Image.open / seek /
 * np.array, one page at a time) for the files it supports: only the file's bytes cross to the device, and the pixels land where the
 * _dev entry points read them.  The file is untrusted: every offset, count and product is checked against its size.
 *
 * tmat_tiff_probe walks the IFD chain of a classic TIFF (II or MM) in host memory; no handle, no GPU.  It fills
 * pages[0, min(cap_pages, *n_pages)) and sets *n_pages to the number of pages found.  status per page:
 *   TMAT_TIFF_OK        the device path decodes it: strips, SamplesPerPixel 1, BitsPerSample 8 or 16, SampleFormat 1 or absent,
 *                       Photometric 1, FillOrder 1, PlanarConfiguration 1 or absent, Compression 1 (none), 5 (LZW, MSB first) or 32773
 *                       (PackBits), Predictor 1, or 2 with LZW, and every strip inside the file
 *   TMAT_TIFF_FALLBACK  a valid file of another kind (reason TMAT_TIFF_R_BIGTIFF and above): the caller decodes it as before
 *   TMAT_TIFF_CORRUPT   inconsistent (reason below TMAT_TIFF_R_BIGTIFF).  Damage to the header or to the chain itself (an IFD outside the
 *                       file, an entry count that overruns it, a chain that loops) ends the walk with one last page of this status
 * A NULL file or a NULL n_pages, cap_pages < 0, or pages NULL with cap_pages > 0: TMAT_E_ARG.
 *
 * The decode calls take planes: plane i is page page_of[i] of file file_of[i] (files[k] with n_bytes[k] bytes, host memory).  All
 * planes of a call have one shape (H, W) and one bit depth; the output is (n_planes, H, W) uint16, 8-bit samples widened, and *bits
 * says 8 or 16 (0 when no plane decoded) for the callers' input_bits.  status[i] is the plane's: a plane that is not TMAT_TIFF_OK --
 * not supported, a page the file does not have, or a strip whose stream turns out corrupt while it is decoded -- leaves its output
 * slice untouched and does not fail the call.  A supported plane of another shape, or two of different depth: TMAT_E_ARG.
 * Stream rules (csrc/tiff.h): LZW codes of 9 to 12 bits read MSB first, widened when the next free entry is (1 << width) - 1, Clear
 * 256, EOI 257, a code equal to the next free entry is the previous string plus its first byte and a code above it is corrupt, a full
 * table (4096) stops growing, a strip ends when rows W bytes are produced and EOI or the end of the input before that is corrupt;
 * PackBits with the same count rules; then byte swap (MM), predictor 2 per row modulo 2^bits, widen.
 * tmat_host_tiff_decode_batch is the host twin (no handle, no GPU); tmat_tiff_decode_batch decodes on the device into host memory,
 * tmat_tiff_decode_batch_dev into out_dev, a tmat_dev_alloc block of n_planes H W uint16.  All three give the same pixels and status.
 * A handle from tmat_create_plain is enough; device memory comes from the handle's pool on first use, in chunks of bounded size.
 */
#define TMAT_TIFF_OK 0
#define TMAT_TIFF_FALLBACK 1
#define TMAT_TIFF_CORRUPT 2
#define TMAT_TIFF_R_NONE 0
#define TMAT_TIFF_R_HEADER 1        /* not a TIFF header, or shorter than one */
#define TMAT_TIFF_R_IFD 2           /* an IFD position or entry count outside the file */
#define TMAT_TIFF_R_LOOP 3          /* the IFD chain returns to an IFD it has visited */
#define TMAT_TIFF_R_TAG 4           /* a needed tag is missing, of a wrong type, or its values lie outside the file */
#define TMAT_TIFF_R_STRIPS 5        /* strip tables inconsistent with the height, or a strip outside the file */
#define TMAT_TIFF_R_STREAM 6        /* reserved for a strip stream found corrupt while decoding (the decode calls report status only) */
#define TMAT_TIFF_R_PAGE 7
#define TMAT_TIFF_R_BIGTIFF 20
#define TMAT_TIFF_R_TILES 21
#define TMAT_TIFF_R_SAMPLES 22      /* SamplesPerPixel other than 1 (RGB, interleaved) */
#define TMAT_TIFF_R_BITS 23         /* BitsPerSample other than 8 or 16 */
#define TMAT_TIFF_R_SAMPLE_FORMAT 24
#define TMAT_TIFF_R_PHOTOMETRIC 25
#define TMAT_TIFF_R_FILL_ORDER 26
#define TMAT_TIFF_R_PLANAR 27
#define TMAT_TIFF_R_COMPRESSION 28  /* Deflate, JPEG, ... */
#define TMAT_TIFF_R_PREDICTOR 29    /* predictor 3, or 2 without LZW */
#define TMAT_TIFF_R_OLD_LZW 30      /* old-style LZW stream (first byte 0, low bit of the second set) */
#define TMAT_TIFF_R_SIZE 31         /* a plane above 2^30 bytes */
typedef struct tmat_tiff_page {
    int32_t width, height, bits, compression, predictor, big_endian, rows_per_strip, n_strips, status, reason;
} tmat_tiff_page;
int tmat_tiff_probe(const uint8_t *file, size_t n_bytes, int cap_pages, tmat_tiff_page *pages, int *n_pages);
int tmat_host_tiff_decode_batch(const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of, int n_planes,
                                int H, int W, uint16_t *out, int *bits, int *status);
int tmat_tiff_decode_batch(tmat_handle h, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of,
                           int n_planes, int H, int W, uint16_t *out_host, int *bits, int *status);
int tmat_tiff_decode_batch_dev(tmat_handle h, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of,
                               int n_planes, int H, int W, void *out_dev, int *bits, int *status);
/* tmat_tiff_decode_batch_dev that also reports ms2 = HIP-event milliseconds on the handle's stream of {upload of the file bytes and the
 * strip tables, kernels} (tools/bench_tiff.py) */
int tmat_tiff_decode_batch_dev_timed(tmat_handle h, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of,
                                     int n_planes, int H, int W, void *out_dev, int *bits, int *status, float *ms2);

/* One result row per image, the payload gathered across ranks. */
typedef struct tmat_row {
    int64_t index;   /* image index in the run                      */
    int64_t count;   /* Total # of branches                         */
    double total_px; /* total branch length in 384-wide pixels      */
    double avg_px;   /* average branch length in 384-wide pixels    */
} tmat_row;

/*
 * The whole per-image compute of analyze_img's 2-D branch (compute_branches.py:307-361, 391-426,
 * 455-457) for a batch with inputs ALREADY RESIDENT IN HBM: imgs_dev (n, H, W) u16 device pointer.
 * rows: n host records (index field = first_index + i).  graph_thresh_1/2, smoothing_window_px,
 * min_branch_length_px, max_branch_length_px (<=0: none), remove_isolated: as computed at
 * compute_branches.py:401-426.
 */
int tmat_analyze_batch_dev(tmat_handle h, const uint16_t *imgs_dev, int n, int H, int W, double ds_ratio,
                           int ds_width, float graph_thresh_1, float graph_thresh_2, int smoothing_window_px,
                           int min_branch_length_px, int max_branch_length_px, int remove_isolated,
                           int64_t first_index, tmat_row *rows);

/* host-pointer convenience wrapper of the above (uploads imgs first) */
int tmat_analyze_batch(tmat_handle h, const uint16_t *imgs, int n, int H, int W, double ds_ratio, int ds_width,
                       float graph_thresh_1, float graph_thresh_2, int smoothing_window_px,
                       int min_branch_length_px, int max_branch_length_px, int remove_isolated,
                       int64_t first_index, tmat_row *rows);

/*
 * tmat_analyze_batch with well masks: the --detect-well form of the 2-D branch (compute_branches.py:318-337, 359-361, 425) through the
 * same two-stage pipeline.  well_masks (n, h, w) u8 host or NULL, (h, w) = (round(W ds_ratio), round(H ds_ratio)) the down-sampled
 * shape: non-zero = inside the well.  They multiply the rescaled image in front of the network (:328, before the input normalisation)
 * and the thresholded mask in front of filter_branch_seg_mask (:334); the centre-line weighting reads the unmasked prediction (:344).
 * pruning_masks (n, fh, fw) u8 host or NULL, (fh, fw) = round((H, W) ds_width / W) the field shape: MorseGraph's pruning_mask per
 * image (:359-361, :425).  With both NULL the rows are tmat_analyze_batch's.
 */
int tmat_analyze_batch_masked(tmat_handle h, const uint16_t *imgs, int n, int H, int W, double ds_ratio, int ds_width,
                              float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                              int max_branch_length_px, int remove_isolated, int64_t first_index, const uint8_t *well_masks,
                              const uint8_t *pruning_masks, tmat_row *rows);

/*
 * tmat_analyze_batch / tmat_analyze_batch_dev "with tree": the same passes, the same rows bit for bit, and per image the tree overlay
 * picture (compute_branches.py:440-449) and the scaled barcode (:377) out of the batched pipeline.  The host graph stage of a pass runs
 * tmat_morse_tree's code instead of tmat_morse_stats' (one shared core), then the pass's segments are uploaded and rasterised on the
 * handle's third stream (overlay_kernels.hip, one launch set per pass) over the pass's Lanczos-down-sampled u16 image, which is kept in
 * HBM for the call; the overlays are copied back per pass.  scaling factor = down-sampled width / field width (:437).
 * rgb_out (n, vh, vw, 3) u8 with vw = vis_width, vh = round_half_even(vis_width h / w) for the (h, w) = (round(W ds_ratio),
 * round(H ds_ratio)) down-sampled image; bars_out (n, cap_b, 2) f64; n_bars (n).  TMAT_E_CAP when an image has more than cap_b bars.
 * Scratch comes from the handle's tool workspaces, sized on first use; the plain entries allocate and do nothing extra.
 */
int tmat_analyze_batch_tree_dev(tmat_handle h, const uint16_t *imgs_dev, int n, int H, int W, double ds_ratio, int ds_width,
                                float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                                int max_branch_length_px, int remove_isolated, int64_t first_index, tmat_row *rows, int vis_width,
                                uint8_t *rgb_out, double *bars_out, int cap_b, int *n_bars);
int tmat_analyze_batch_tree(tmat_handle h, const uint16_t *imgs, int n, int H, int W, double ds_ratio, int ds_width,
                            float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                            int max_branch_length_px, int remove_isolated, int64_t first_index, tmat_row *rows, int vis_width,
                            uint8_t *rgb_out, double *bars_out, int cap_b, int *n_bars);

/*
 * The extensible form of the entries above: one call that carries any combination of their requests, and the stage pictures.  The
 * rows are those of the matching entry above, bit for bit, for every combination.
 *   size                          sizeof(tmat_analyze_opts) as the caller compiled it; TMAT_E_ARG for a size this library does not know
 *   ds_ratio .. first_index       as tmat_analyze_batch_dev (compute_branches.py:309-312, 401-426)
 *   well_masks, pruning_masks     as tmat_analyze_batch_masked (:318-337, :359-361, :425), host pointers, either may be NULL
 *   vis_width .. n_bars           as tmat_analyze_batch_tree (:431-450); rgb_out NULL: no tree, the other four are not read.  With masks
 *                                 as well, the overlay is the PRUNED graph's tree over the u16 down-sampled (unmasked) image
 *   stage_out                     NULL, or (n, 4, h, w) u8 host, (h, w) = (round(W ds_ratio), round(H ds_ratio)): save_vis (see
 *                                 tmat_stage_pictures) of the four arrays the reference dumps, taken from the pass's buffers in HBM --
 *                                 plane TMAT_STAGE_ORIGINAL the Lanczos-down-sampled image before any well mask (:312-315),
 *                                 _PREDICTION the network's prediction, of the masked input when there are well masks (:328-331),
 *                                 _MASK the filtered segmentation mask (:334-337, :347), _WEIGHTED the centre-line weighted prediction
 *                                 (:341-344, :348 distance_transform.png).  Copied back per pass.
 * Scratch for the tree and the pictures comes from the handle's tool workspaces, sized on first use; a call without them allocates and
 * does nothing extra.  tmat_analyze_batch_ex takes host images, tmat_analyze_batch_ex_dev images ALREADY RESIDENT IN HBM.
 */
#define TMAT_STAGE_ORIGINAL 0
#define TMAT_STAGE_PREDICTION 1
#define TMAT_STAGE_MASK 2
#define TMAT_STAGE_WEIGHTED 3
typedef struct tmat_analyze_opts {
    uint32_t size;
    double ds_ratio;
    int ds_width;
    float graph_thresh_1, graph_thresh_2;
    int smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated;
    int64_t first_index;
    const uint8_t *well_masks, *pruning_masks;
    int vis_width;
    uint8_t *rgb_out;
    double *bars_out;
    int cap_b;
    int *n_bars;
    uint8_t *stage_out;
} tmat_analyze_opts;
int tmat_analyze_batch_ex(tmat_handle h, const uint16_t *imgs, int n, int H, int W, const tmat_analyze_opts *o, tmat_row *rows);
int tmat_analyze_batch_ex_dev(tmat_handle h, const uint16_t *imgs_dev, int n, int H, int W, const tmat_analyze_opts *o, tmat_row *rows);

/*
 * The grid form of the extensible entry: graph_thresh_1 / graph_thresh_2 as lists (compute_branches.py:366-395, the parameter-tuning
 * mode).  The reference analyses an image once and builds one MorseGraph per pair from the same field (:391-426); so does this call:
 * every pass of the network, the filter, the thinning, the finish stage and the DMT front end runs ONCE, and only the tail that reads
 * the thresholds (`collect`, then tmat_morse_stats / tmat_morse_tree) runs per pair, on the host workers over (pair, image).
 *   size            sizeof(tmat_grid_opts) as the caller compiled it; TMAT_E_ARG for a size this library does not know
 *   n_thresh, thresh   n_thresh >= 1 pairs (graph_thresh_1, graph_thresh_2), host, as tmat_stack_opts; o->graph_thresh_1 / _2 are not read
 *   rows            (n_thresh, n): rows[t n + i] is image i at pair t -- bit for bit the row of tmat_analyze_batch_ex at that pair with
 *                   the same masks
 *   o->rgb_out, o->bars_out, o->n_bars   gain a leading n_thresh axis: (n_thresh, n, vh, vw, 3), (n_thresh, n, cap_b, 2), (n_thresh, n);
 *                   each slice holds the bytes of tmat_analyze_batch_tree at that pair.  o->stage_out keeps (n, 4, h, w): the stage
 *                   pictures do not depend on the pair.  TMAT_E_CAP when any (t, i) has more than cap_b bars
 *   tree_png        NULL, or room for (n_thresh, n) files of tree_png_cap bytes each: the same overlays as complete PNG files, encoded
 *                   on the device from the raster in HBM (png_kernels.hip); file (t, i) at tree_png + (t n + i) tree_png_cap for
 *                   tree_png_sizes[t n + i] bytes, the bytes of tmat_png_encode_batch of the raw overlay; bytes behind a file are not
 *                   written.  o->rgb_out may then be NULL -- no raw overlay crosses to the host --; vis_width, bars_out, cap_b and n_bars
 *                   are still read.  tree_png_cap below tmat_png_bound(vh, vw, 3): TMAT_E_CAP before any pass starts
 *   barcode_png     NULL, or the same for the barcode picture of (t, i): rasterised on the device from that pair's scaled bars
 *                   (tmat_render_barcode), then encoded; the bytes of tmat_host_png_encode_batch(tmat_host_render_barcode(bars)).  Its
 *                   bound is tmat_png_bound(S, S, 3), S = round_half_even(0.9 vis_width).  It takes the tree request's vis_width,
 *                   bars_out, cap_b and n_bars, since the bars come from it
 * TMAT_E_ARG: n_thresh < 1, thresh NULL, an unknown size of either struct, a handle from tmat_create_plain; nothing is then written.
 * Scratch comes from the handle's tool workspaces, sized on first use.  The picture buffers grow with n_thresh: callers bound the
 * images per call (tmat_amd/branches.py:grid_images_per_call).
 */
typedef struct tmat_grid_opts {
    uint32_t size;
    int n_thresh;
    const float *thresh;
    uint8_t *tree_png;
    size_t tree_png_cap;
    size_t *tree_png_sizes;
    uint8_t *barcode_png;
    size_t barcode_png_cap;
    size_t *barcode_png_sizes;
} tmat_grid_opts;
int tmat_analyze_batch_grid(tmat_handle h, const uint16_t *imgs, int n, int H, int W, const tmat_analyze_opts *o, const tmat_grid_opts *g,
                            tmat_row *rows);
int tmat_analyze_batch_grid_dev(tmat_handle h, const uint16_t *imgs_dev, int n, int H, int W, const tmat_analyze_opts *o,
                                const tmat_grid_opts *g, tmat_row *rows);

/* ---------------------------------------------------------------------------------------------------------------
 * Z-stack (Sato) branch of analyze_img: reference scripts/compute_branches.py:224-306 (csrc/sato_kernels.hip,
 * csrc/stack_pipeline.cpp).  Its arithmetic lives in scikit-image / scipy.ndimage (reference setup.py pins
 * scikit-image==0.22.0, scipy==1.13.1); oracle/sato.py restates it.  A handle from tmat_create_plain is enough.
 * --------------------------------------------------------------------------------------------------------------- */

/* Hessian of skimage.filters.sato: 0 = gaussian derivatives (scikit-image >= 0.20, what the pinned 0.22.0 runs:
 * hessian_matrix(use_gaussian_derivatives=True), -image, vesselness sigma^2 * max(l1, 0));  1 = gradient of the smoothed
 * image (scikit-image <= 0.19: gaussian, np.gradient twice, 1 - image, sigma^2-scaled elements). */
#define TMAT_SATO_GAUSSIAN_DERIVATIVES 0
#define TMAT_SATO_GRADIENT 1
/* scipy.ndimage boundary modes of tmat_gaussian_f32 */
#define TMAT_EXT_NEAREST 0
#define TMAT_EXT_REFLECT 1
#define TMAT_EXT_MIRROR 2

/*
 * Replace the kernel table of scipy's gaussian_filter1d for (sigma, order, radius) on this handle: weights = the 2 radius + 1
 * values scipy hands to correlate1d (ndimage/_filters.py:_gaussian_kernel1d(sigma, order, radius)[::-1]).  Without it the
 * library forms the table with libm's exp; numpy's exp is CPU-dispatched and differs from libm in the last bit at some taps,
 * so a host that wants scipy's exact results on its machine hands over numpy-made tables (tmat_amd/sato.py does).
 */
int tmat_set_gaussian_table(tmat_handle h, double sigma, int order, int radius, const double *weights);
/* the library's own table (host only): scipy's formula with libm's exp and numpy's pairwise sum; order 0 or 1 */
int tmat_host_gaussian_kernel1d(double sigma, int order, int radius, double *weights);

/* skimage.filters.gaussian(x, sigma, mode) on a float32 array (d0, d1, d2) (= ndi.gaussian_filter, truncate 4, f64
 * accumulation, f32 after every axis); d0 = 1 filters a 2-D image (d1, d2).  compute_branches.py:248, 269, 282, 302 */
int tmat_gaussian_f32(tmat_handle h, const float *x, int d0, int d1, int d2, double sigma, int mode, float *out);

/* skimage.filters.sato(img, sigmas, black_ridges=False) on n float32 images (n, h, w) (compute_branches.py:261-263) */
int tmat_sato_batch(tmat_handle h, const float *imgs, int n, int hh, int ww, const double *sigmas, int n_sigmas, int hessian,
                    float *out);

/* compute_branches.py:247-256: per-slice gaussian written back into the integer stack, skimage resize of the stack to
 * (Z, out_h, out_w) (order 1, anti-aliased, preserve_range), rescale_intensity(0..1) over the stack.
 * stack (Z, H, W) u16 host (8-bit stacks widened); vol (Z, out_h, out_w) f32 host. */
int tmat_stack_prepare(tmat_handle h, const uint16_t *stack, int Z, int H, int W, int out_h, int out_w, float *vol);

/* optional host copies of the stages of tmat_vessel_field (any member may be NULL) */
typedef struct tmat_vessel_stages {
    float *vess;       /* (Z-1, h, w) Sato response of every slice pair          :258-266 */
    float *sharp;      /* (Z-1, h, w) unsharp_mask(vess, 2, 2)                   :269     */
    float *vessels;    /* (h, w) its max projection                               :270     */
    uint8_t *edges;    /* (h, w) canny(vessels, sigma=0)                          :271     */
    uint8_t *skel;     /* (h, w) medial_axis(edges)                               :274     */
    uint8_t *mask_sel; /* (h, w) components with eccentricity * diameter > 3.5    :276-279 */
    uint8_t *grown;    /* (h, w) after the 10 region-growing rounds               :283-294 */
    uint8_t *closed;   /* (h, w) closing(mask & ~edges, disk(2))                  :296-297 */
    uint8_t *filt;     /* (h, w) filter_branch_seg_mask(closed, None, False)      :299     */
} tmat_vessel_stages;

/* compute_branches.py:258-302: prepared stack vol (Z, h, w) f32 in 0..1 -> vesselness image field (h, w) f32 */
int tmat_vessel_field(tmat_handle h, const float *vol, int Z, int hh, int ww, int hessian, float *field,
                      const tmat_vessel_stages *stages);

/*
 * The whole per-image compute of analyze_img for a Z stack (compute_branches.py:224-306, 391-426, 455-457; no well
 * mask): stack (Z, H, W) u16 host -> one result row.  The field is (round(H ds_width / W), ds_width); the graph
 * parameters are those of tmat_analyze_batch.  field_out (nullable) receives the vesselness image.
 * The device blocks a Z-stack call allocates (this and the stage-wise entry points above) go back to a pool on the handle
 * when it returns and are taken from there by the next call; tmat_destroy frees the pool.
 */
int tmat_analyze_stack(tmat_handle h, const uint16_t *stack, int Z, int H, int W, int ds_width, int hessian,
                       float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                       int max_branch_length_px, int remove_isolated, int64_t index, tmat_row *row, float *field_out);

/* The common tail of analyze_img from a vesselness image (compute_branches.py:391-426, 455-457): rescale to 0..255, DMT
 * graph, MorseGraph statistics -> one row.  field (fh, fw) f32 host.  Lets a host that sweeps the graph_thresh grid
 * (:366-395) compute the field once. */
int tmat_field_stats(tmat_handle h, const float *field, int fh, int fw, float graph_thresh_1, float graph_thresh_2,
                     int smoothing_window_px, int min_branch_length_px, int max_branch_length_px, int remove_isolated,
                     int64_t index, tmat_row *row);

/* The same with MorseGraph's pruning_mask (topology.py: branches that end inside the mask are trimmed): the Z-stack
 * branch with --detect-well passes the inverse of the shrunken well mask (compute_branches.py:243, 412-420).
 * pruning_mask (fh, fw) u8 host, nonzero = prune; NULL = none. */
int tmat_field_stats_pruned(tmat_handle h, const float *field, int fh, int fw, float graph_thresh_1, float graph_thresh_2,
                            int smoothing_window_px, int min_branch_length_px, int max_branch_length_px, int remove_isolated,
                            const uint8_t *pruning_mask, int64_t index, tmat_row *row);

/*
 * Batch form of the Z-stack branch.  n stacks of one shape (n, Z, H, W) u16 host go through the device stages in
 * passes of K stacks, one launch set per pass (every per-image quantity -- extrema, labels, borders -- stays per stack); while the
 * device works on pass p, a host thread runs the graph stage of pass p - 1 (DMT collect + MorseGraph statistics per stack and
 * threshold pair, on the worker threads TMAT_HOST_THREADS sizes).  The field never leaves HBM between the stages, and the whole
 * threshold grid (compute_branches.py:366-395) is swept from it.
 * K = min(n, TMAT_STACK_PASS_MAX, TMAT_STACK_PASS_BUDGET / device bytes of one stack), at least 1; the bytes are summed over the
 * blocks a pass takes (the three Z H W f64 planes of the resize dominate).  The budget is a fixed cap, not a tuned number.
 * opts.pass_stacks > 0 overrides K.  tmat_stack_pass_plan (host only) reports K and the bytes for a geometry.
 */
#define TMAT_STACK_PASS_MAX 8
#define TMAT_STACK_PASS_BUDGET (8ull << 30)   /* 8 GiB of device memory per pass */
typedef struct tmat_stack_opts {
    uint32_t size;                       /* sizeof as the caller compiled it; TMAT_E_ARG if unknown */
    int ds_width, hessian;
    int n_thresh; const float *thresh;   /* n_thresh pairs (graph_thresh_1, graph_thresh_2)          */
    int smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated;
    int64_t first_index;
    const uint8_t *pruning_masks;        /* NULL or (n, fh, fw) u8 host, as tmat_field_stats_pruned  */
    float *fields_out;                   /* NULL or (n, fh, fw) f32 host                              */
    uint8_t *proj_pic_out;               /* NULL or (n, H, W) u8: save_vis of the max projection      */
    uint8_t *field_pic_out;              /* NULL or (n, fh, fw) u8: save_vis of the field             */
    int pass_stacks;                     /* 0 = automatic                                             */
    /* -- the first version of the struct (TMAT_STACK_OPTS_SIZE_V1) ended here; what follows is the tree request, all zero = none -- */
    int vis_width;                       /* canvas width of the overlays (--vis-width)                */
    uint8_t *rgb_out;                    /* NULL or (n_thresh, n, vh, vw, 3) u8 host: the overlays    */
    double *bars_out;                    /* (n_thresh, n, cap_b, 2) f64 host: [birth, death] * W / fw */
    int cap_b;                           /* bars a (pair, stack) item may have                        */
    int *n_bars;                         /* (n_thresh, n) host: bars of every item                    */
} tmat_stack_opts;
/* sizeof(tmat_stack_opts) before the tree request was added.  A caller that passes it in `size` is served as before: the fields up to
 * pass_stacks are read, nothing behind them. */
#define TMAT_STACK_OPTS_SIZE_V1 88u
/* compute_branches.py:224-306, 366-395, 391-426 for n stacks: rows (n_thresh, n), rows[t * n + i] = stack i at threshold pair t, equal
 * to tmat_analyze_stack (or tmat_field_stats_pruned with the stack's pruning mask) at that pair bit for bit, whatever K is.  The two
 * pictures (:228-229 original_image.png, :303 vesselness_image.png) are the bytes tmat_stage_pictures gives for the stack's max
 * projection and for its field, rendered from the buffers in HBM.
 * Tree request (compute_branches.py:431-450; the fields mean what they mean in tmat_analyze_opts for tmat_analyze_batch_grid, each with
 * a leading n_thresh axis): with bars_out (and n_bars, cap_b) the host graph stage calls tmat_morse_tree for every (pair, stack) with
 * the stack's pruning mask and the scaling factor W / fw -- the row comes out of the same call and equals the row without a request --
 * and item (t, i) leaves its bars at bars_out + (t n + i) cap_b 2 and their count in n_bars[t n + i].  With rgb_out as well, a pass
 * keeps the u16 max projections of its stacks in HBM (taken before the per-slice gaussian) and the overlays are rasterised over them
 * (tmat_render_tree's picture, bg_dtype u16) on a vis_width x round_half_even(vis_width H / W) canvas: the bytes of
 * tmat_host_render_tree for the host's max projection and tmat_morse_tree's segments.  The rasteriser runs on the handle's stream in
 * order with the passes' stages, never beside them.  TMAT_E_CAP: cap_b is too small for some item (n_bars holds what the items that
 * ran need); TMAT_E_ARG: bars_out without n_bars, cap_b < 0, rgb_out without bars_out or with an empty canvas. */
int tmat_analyze_stack_batch(tmat_handle h, const uint16_t *stacks, int n, int Z, int H, int W,
                             const tmat_stack_opts *o, tmat_row *rows /* (n_thresh, n) */);
/* The same for stacks that are already in device memory: stacks_dev (n, Z, H, W) u16 from tmat_dev_alloc / tmat_dev_upload.  A pass
 * copies its K stacks device to device into the block the per-slice gaussian overwrites; the caller's buffer is only read and holds
 * after the call what it held before.  Rows, fields and pictures are those of the host-pointer form bit for bit, whatever K. */
int tmat_analyze_stack_batch_dev(tmat_handle h, const uint16_t *stacks_dev, int n, int Z, int H, int W,
                                 const tmat_stack_opts *o, tmat_row *rows /* (n_thresh, n) */);
/* compute_branches.py:258-302 for n prepared stacks vols (n, Z, h, w) in one launch set -> fields (n, h, w); the arrays of `stages`
 * carry a leading n */
int tmat_vessel_field_batch(tmat_handle h, const float *vols, int n, int Z, int hh, int ww, int hessian,
                            float *fields, const tmat_vessel_stages *stages /* arrays with leading n */);
/* stacks per pass and device bytes per stack of tmat_analyze_stack_batch for n stacks of (Z, H, W) (either output may be NULL) */
int tmat_stack_pass_plan(int n, int Z, int H, int W, int ds_width, int pass_stacks, int *stacks_per_pass,
                         uint64_t *bytes_per_stack);
/* Measurement aid (tools/bench_stack.py): per pass of the handle's last tmat_analyze_stack_batch, the wall milliseconds of its device
 * stages (upload to the copy back of the DMT outputs) and of its host graph stage.  n_pass = passes of that call; at most cap are written. */
int tmat_debug_stack_trace(tmat_handle h, int cap, int *n_pass, double *gpu_ms, double *host_ms);

/* skimage.transform.resize(x, (n, out_h, out_w), order=1, preserve_range=True, anti_aliasing=True) of n integer images
 * (scikit-image >= 0.19: anti-aliasing gaussian + grid-mode linear zoom, clipped to the input's range), float64 out.
 * compute_branches.py:232-238 resizes the max projection of a Z stack with it before make_well_mask.
 * imgs (n, H, W) u16 host (8-bit images widened); out (n, out_h, out_w) f64 host. */
int tmat_resize_aa_u16(tmat_handle h, const uint16_t *imgs, int n, int H, int W, int out_h, int out_w, double *out);

/* ---------------------------------------------------------------------------------------------------------------
 * Cell-area tool: reference scripts/compute_cell_area.py:29-87, 164-178 and
 * fl_tissue_model_tools/preprocessing.py:44-93 (csrc/cellarea_kernels.hip).  A handle from tmat_create_plain is enough.
 * --------------------------------------------------------------------------------------------------------------- */

/*
 * For n uint16 images (n, H, W) (Z stacks: project first, tmat_zproj_batch method max): cv2.resize to (out_h, out_w)
 * with bilinear interpolation (compute_cell_area.py:57 passes INTER_AREA in the position of `dst`, so the default
 * interpolation applies; out_h = out_w = 0: no resize), rescale_intensity to 0..1 as float32 (:79),
 * preprocessing.exec_threshold (:44-93: two-component gaussian mixture of the pixel intensities -- fitted here to the
 * intensity histogram, from the optimal 2-means partition, with scikit-learn's EM update and stopping rule -- and the
 * threshold foreground mean + sd_coef * foreground sd), compute_area_prop (:164-178).
 * area: n fractions of pixels kept.  thresholded (nullable): (n, out_h, out_w) u8, 255 where kept (:87).
 * params (nullable): n x 9 doubles [threshold, weight0, weight1, mean0, mean1, var0, var1, EM iterations, converged].
 * The call's device workspaces (sized by the largest batch seen) stay on the handle until tmat_destroy: the reference's
 * default batch is 4 images, for which a hipMalloc / hipFree pair per buffer and call cost more than the kernels.
 * tmat_inv_depth_predict keeps its workspaces the same way.
 */
int tmat_cell_area_batch(tmat_handle h, const uint16_t *imgs, int n, int H, int W, int out_h, int out_w, double sd_coef,
                         double *area, uint8_t *thresholded, double *params);

/*
 * The --detect-well form of the same tool (compute_cell_area.py:117-130, 273-286; preprocessing.exec_threshold with
 * mask_idx): imgs (n, H, W) u16 are the ALREADY down-sampled images, masks (n, H, W) u8 their well masks
 * (well_mask_generation.generate_well_mask(img, mask_val=255) > 0).  rescale_intensity uses the extrema of the whole image,
 * the mixture is fitted to the pixels inside the mask only, pixels outside count as background.  area[i] = kept pixels /
 * (H W): the caller divides by the well's pixel count (compute_area_prop with well_pix_area).
 * tmat_resize_linear_u16 = the down-sampling step alone (compute_cell_area.py:54-57, cv2.resize with the default
 * INTER_LINEAR; exactly halving both axes takes cv2's INTER_AREA shortcut (a + b + c + d + 2) >> 2): imgs (n, H, W) ->
 * out (n, out_h, out_w), host buffers.
 */
int tmat_cell_area_masked(tmat_handle h, const uint16_t *imgs, const uint8_t *masks, int n, int H, int W, double sd_coef, double *area,
                          uint8_t *thresholded, double *params);
int tmat_resize_linear_u16(tmat_handle h, const uint16_t *imgs, int n, int H, int W, int out_h, int out_w, uint16_t *out);

/*
 * Max projection and down-sampling of n Z stacks in one kernel (compute_cell_area.py:50-57: img.max(0), then cv2.resize), for
 * stacks that are resident in device memory: src_dev (n, Z, H, W) u16 (tmat_dev_alloc; 8-bit sources widened), read only ->
 * small_dev (n, out_h, out_w) u16, device.  Every output pixel takes the maximum over Z of each of its source taps and then the
 * arithmetic of tmat_resize_linear_u16 on those maxima: the float bilinear form (src_bits 16), cv2's fixed-point form (src_bits 8),
 * the integer 2 x 2 mean when H == 2 out_h && W == 2 out_w.  The full-resolution projection is never written and only the rows
 * the taps touch are read.  Z == 1 is tmat_resize_linear_u16 without the copies.  out_h = out_w = 0: the plain max projection,
 * small_dev (n, H, W).  src_bits is explicit: tmat_set_input_depth is not read.
 * Z >= 1, n <= 65535, H W <= 2^30, src_bits 8 or 16, out_h / out_w both 0 or both positive: TMAT_E_ARG otherwise, nothing written.
 * Returns after the kernel has run.
 */
int tmat_cell_small_dev(tmat_handle h, const uint16_t *src_dev, int n, int Z, int H, int W, int src_bits, int out_h, int out_w,
                        uint16_t *small_dev);

/*
 * The tail of tmat_cell_area_batch / tmat_cell_area_masked (rescale_intensity, mixture fit, threshold, area: compute_cell_area.py:79-87,
 * preprocessing.py:44-93) on images that are already down-sampled and resident: small_dev (n, hh, ww) u16 device, read only.
 * masks: host, NULL (the unmasked form of tmat_cell_area_batch) or (n, hh, ww) u8 with the meaning of tmat_cell_area_masked (extrema
 * of the whole image, mixture inside the mask, area[i] = kept pixels / (hh ww)).  area, thresholded (nullable, (n, hh, ww) u8) and
 * params (nullable, n x 9) are host buffers as there; the three entry points run the same code from here on.  n <= 65535.
 */
int tmat_cell_area_fit_dev(tmat_handle h, const uint16_t *small_dev, const uint8_t *masks, int n, int hh, int ww, double sd_coef,
                           double *area, uint8_t *thresholded, double *params);

/* ---------------------------------------------------------------------------------------------------------------
 * Invasion-depth tool: reference scripts/compute_inv_depth.py:96-172, models.py:33-82 (build_ResNet50_TL),
 * data_prep.py:17-61 (csrc/resnet_kernels.hip; the 1x1 / 3x3 convolutions run on the conv_mfma_kernel of the branching
 * path).  A handle from tmat_create_plain is enough.
 * --------------------------------------------------------------------------------------------------------------- */

/* One classifier = keras.applications ResNet50 up to a `conv{N}_block{K}_out` layer + GlobalAveragePooling2D + Dense(1) +
 * sigmoid.  weights_blob: "TMATW001" container (tmat_amd/inv_depth.py:pack_resnet) with Keras layouts -- conv1.{w,b,bn},
 * s{stage}b{block}.c{1,2,3}.{w,b,bn} (+ .c0 for the projection shortcut of block 1), fc.{w,b}; bn = (4, C) gamma, beta,
 * moving mean, moving variance, eps 1.001e-5.  Returns the model's id on this handle. */
int tmat_resnet_load(tmat_handle h, const void *weights_blob, size_t n_bytes, int *model_id);
/* model.predict(x): x (n, size, size, 3) float32 host (already preprocessed), prob (n) float32.  size % 32 == 0 */
int tmat_resnet_predict(tmat_handle h, int model_id, const float *x, int n, int size, float *prob);
/* compute_inv_depth.py:150-156 for one Z stack: data_prep.prep_inv_depth_imgs (cv2.resize to size x size -- bilinear: the
 * interpolation argument sits in the position of `dst` --, rescale_intensity 0..255, three identical channels,
 * resnet50.preprocess_input) and every model's prediction per slice.  stack (Z, H, W) u16 host; probs (Z, n_models);
 * x_out (nullable): the prepared input (Z, size, size, 3) f32. */
int tmat_inv_depth_predict(tmat_handle h, const int *model_ids, int n_models, const uint16_t *stack, int Z, int H, int W,
                           int size, float *probs, float *x_out);
/* The same for n_stacks Z stacks of one (H, W) in ONE call (compute_inv_depth.py:123-166 loops over the stacks; every step is per
 * slice, so stacks ride together through the classifiers): stacks[k] (Zs[k], H, W) u16 host -- uploaded back to back, no
 * concatenation on the host --, probs (sum of Zs, n_models) in stack order. */
int tmat_inv_depth_predict_multi(tmat_handle h, const int *model_ids, int n_models, const uint16_t *const *stacks, const int *Zs,
                                 int n_stacks, int H, int W, int size, float *probs);

/*
 * Arithmetic of the classifier's convolutions (the 40 trunk convolutions and the im2col stem convolution of every model).
 *   TMAT_RESNET_PRECISION_F32 (default) f32 operands on v_mfma_f32_32x32x2_f32: bit-exact with oracle/resnet.py.
 *   TMAT_RESNET_PRECISION_F16 opt-in: in each of those convolutions the input activation and the weight are each rounded ONCE to
 *       IEEE binary16, round to nearest even, magnitudes above 65504 saturating to +-65504 (never inf / NaN; f16 subnormals are
 *       kept, the matrix instruction does not flush them); products exact; accumulation in f32 on v_mfma_f32_32x32x16_f16 in a
 *       fixed order (same input -> same bits, call after call); everything behind the accumulator is the f32 code of the default
 *       mode (fmaf(acc, scale, shift), residual add, ReLU) and activations stay f32 in memory.  Data preparation, im2col,
 *       max-pool, global average, dense unit and sigmoid are unchanged.  NOT bit-exact with oracle/resnet.py: on synthetic
 *       ensembles a member's probability moves by up to ~2e-3 and the ensemble mean by a few 1e-4, so the 4th decimal of the
 *       printed probability changes on most slices (DESIGN 7c has the measured figures; fine-tuned checkpoints are unmeasured).
 *   TMAT_RESNET_PRECISION_F16ACT opt-in: the f16 mode with every activation tensor of the classifier -- the im2col tensor, the stem
 *       output, the pool output, every trunk convolution's output, the shortcut -- living in memory as IEEE binary16.  Weights: the
 *       same single f16 plane as the f16 mode.  im2col rounds the prepared f32 input ONCE (nearest even, magnitudes above 65504
 *       saturating to +-65504).  A convolution multiplies the stored f16 values as they are (no further rounding), accumulates in f32
 *       on v_mfma_f32_32x32x16_f16 with the f16 mode's k-step geometry and order (a k step = 16 consecutive channels of one tap, a
 *       lane half carrying 8 of them; per accumulator: 32-channel blocks ascending, inside a block tap-major, k steps ascending --
 *       on the same f16-exact operands the accumulator equals the f16 mode's bit for bit), runs the f32 epilogue
 *       (fmaf(acc, scale, shift), + the residual, an f16 value widened exactly, ReLU) and rounds the result ONCE to f16 with the
 *       same rounding and saturation before it is stored.  Max-pool takes the maximum of f16 values (exact); global average, dense
 *       unit and sigmoid are the f32 code of the other modes reading widened f16.  Data preparation is unchanged.  The activation
 *       buffers of the other modes are reused at half their bytes.  Same input -> same bits, call after call.  NOT bit-exact with
 *       oracle/resnet.py and NOT equal to the f16 mode: every stored activation carries an f16 rounding (DESIGN 7c has the figures).
 * Works on any handle (tmat_create_plain included), independent of tmat_set_precision; drains the handle's streams, then
 * applies to the calls that follow (tmat_resnet_predict, tmat_inv_depth_predict, tmat_inv_depth_predict_multi).  The f16
 * copy of a model's weights is made on the host when a 16-bit mode is first on and freed with the model.  Other values (2
 * included): TMAT_E_ARG.  TMAT_INV_DEPTH_PRECISION=f32|f16|f16act selects the mode at handle creation (any other value fails creation).
 */
#define TMAT_RESNET_PRECISION_F32 0
#define TMAT_RESNET_PRECISION_F16 1
#define TMAT_RESNET_PRECISION_F16ACT 3
int tmat_resnet_set_precision(tmat_handle h, int mode);
/*
 * Stage-wise test entry point: ONE convolution of conv_mfma_kernel on host buffers.  x (n, hh, ww, cin) f32; w in the Keras
 * layout (ksize, ksize, cin, cout); ksize 1 (stride 1 or 2, TF SAME: even indices) or 3 (stride 1, SAME);
 * v = scale ? fmaf(acc, scale, shift) : acc + shift, + resid (nullable, shaped like out), ReLU on load / on store as asked; out
 * (n, hh / stride, ww / stride, cout).  prec 0: the f32 contract (bit-exact with oracle/unet.py:_conv); prec 3: the f16 contract
 * above; prec 4: ONE f16act convolution: x -- after the load-side ReLU -- and resid are rounded to f16 on the host, the convolution
 * runs on f16 device buffers, out is its f16 output widened to f32: round_f16(the prec 3 result on the same f16-exact operands), bit
 * for bit.
 * Accepted shapes, in every precision (what launch_conv checks; tests/test_gpu_conv_shapes.py runs both sides of each):
 *   cin % 64 == 0 (a K loop step is two 32-channel chunks; 32 and 96 are refused);
 *   cout % 64 == 0: 128-wide column tiles when cout % 128 == 0, 64-wide ones otherwise (64, 192, 320, ...; 32 and 96 are refused);
 *   hh and ww multiples of the stride, and an output at least two pixels wide (ww / stride >= 2; one row is fine);
 *   n (hh / stride) (ww / stride) < 2^30.
 * Anything else -- ksize 3 at stride 2 included -- returns TMAT_E_ARG with a message before a kernel is launched.  Any other
 * width, height or pixel count is taken: the prologue is row-uniform for output widths that are multiples of 8 and per-lane
 * otherwise, and the last pixel tile may end past the last pixel.
 */
int tmat_conv2d(tmat_handle h, int prec, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int stride, int cout,
                const float *scale, const float *shift, const float *resid, int relu_in, int relu_out, float *out);
/*
 * Stage-wise test entry point of the REGION form of that kernel (conv_mfma_kernel<..., ROI>, what the tiled entry points launch on the up
 * path): the same contract, f32 only, stride 1, on host buffers, with a segment table.  segs: nseg <= 64 segments of six ints
 * (p0, np, y0, x0, rh, rw), ascending and disjoint in the patches -- or the previous segment's patch range again, with a rectangle
 * disjoint from every other rectangle of that range: the patches [p0, p0 + np) compute the rectangle of rh rows and rw >= 2
 * columns from (y0, x0) of their output and nothing else.  nseg == 0: the full-frame launch of the same convolution.
 *   rs (0 or 1): resid (nullable) is (n, hh >> rs, ww >> rs, cout) and pixel (y, x) adds resid[y >> rs][x >> rs] (hh, ww even for rs 1).
 *   subpixel != 0 (ksize 3, no resid, no out_relu): the 3x3 convolution over the 2x nearest-upsampled x in its sub-pixel form, the weights
 *     pre-summed per output parity class by the function the network's own packing uses; out is (n, 2 hh, 2 ww, cout) and the segments
 *     enumerate STORED pixels (hh x ww): stored pixel (i, j) makes the outputs (2 i + {0, 1}, 2 j + {0, 1}).
 *   out is filled by the CALLER and comes back with the computed pixels replaced: a word outside the rectangles keeps what it held.
 *   out_relu (nullable; caller-filled likewise): the activated copy max(v, +0) that the up path's second convolutions write.
 * Accepted shapes (launch_conv's checks; anything else returns TMAT_E_ARG with a message, launches nothing and leaves out as it was):
 * cin % 64 == 0 for ksize 1 and 3, cin % 32 == 0 for the sub-pixel form (its four taps per class make an even chunk count at 32);
 * cout % 64 == 0 (128-wide column tiles when cout % 128 == 0, 64-wide otherwise); ww >= 2; n hh ww < 2^30; with segments, an output plane
 * per patch below 2^31 bytes.
 * Any first column and any width are taken: the epilogue runs its row-uniform form where a group of 4 or 8 pixels lies in one row, its
 * row-split form on other widths >= 8 and the per-lane form below 8; the prologue is row-uniform for widths that are multiples of 8 and
 * per-lane otherwise.  Inside the rectangles the bits are those of the full-frame launch.
 */
int tmat_conv2d_roi(tmat_handle h, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int subpixel, int cout,
                    const float *scale, const float *shift, const float *resid, int rs, int relu_in, int relu_out, const int *segs, int nseg,
                    float *out, float *out_relu);
/* The same for the 1x1 form at stride 2 (TF SAME samples the even pixels; the down path's residual launches): hh and ww even, no
 * residual, out (and out_relu) (n, hh / 2, ww / 2, cout), the segments' rectangles in output pixels. */
int tmat_conv2d_roi_s2(tmat_handle h, const float *x, int n, int hh, int ww, int cin, const float *w, int cout, const float *scale,
                       const float *shift, int relu_in, int relu_out, const int *segs, int nseg, float *out, float *out_relu);
/*
 * Stage-wise test entry point of the NARROW layers' kernel (csrc/conv_narrow_kernels.hip: what the UNet driver launches for the
 * convolutions conv_mfma_kernel refuses -- the 16- and 32-channel layers of models with filter_counts (32, 64, 128, 256) or
 * (16, 32, 64, 128)): tmat_conv2d_roi's contract on host buffers, with the stride as an argument.  w in the Keras layout; out and
 * out_relu caller-filled; nseg == 0: the full-frame launch; segments as above (stride 2: output pixels, sub-pixel: stored pixels), any
 * first column, any width >= 2.  f32 contract only: bit for bit oracle/unet.py:_conv / _conv_subpixel, and bit for bit conv_mfma_kernel
 * on the shapes both take.
 * Accepted shapes (anything else returns TMAT_E_ARG with "launch_conv_narrow: unsupported shape" or this entry point's own message,
 * launches nothing and leaves out as it was):
 *   cin % 16 == 0 and cout % 16 == 0, both >= 16 (48 and 80 included: a last K block of 16 channels is short, a last column tile half empty);
 *   ksize 3 at stride 1; ksize 1 at stride 1 or 2 (hh and ww even, no resid); subpixel != 0 (ksize 3, stride 1, no resid, no out_relu);
 *   rs 0 or 1 (hh, ww even for rs 1); ww / stride >= 2 (one row is fine); n (hh / stride) (ww / stride) < 2^30.
 * A handle from tmat_create_plain is enough.
 */
int tmat_conv2d_narrow(tmat_handle h, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int stride, int subpixel,
                       int cout, const float *scale, const float *shift, const float *resid, int rs, int relu_in, int relu_out,
                       const int *segs, int nseg, float *out, float *out_relu);
/*
 * Which kernel every convolution of a weight blob runs on.  Host arithmetic: no GPU, no handle.  layers (cap, 6) i32 receives, in the
 * launch order of one forward (down path, then up path), [ksize, stride, cin, cout, output side, launcher] per convolution launch:
 * ksize 2 is the sub-pixel form; a 1x1 over the stem at its even pixels counts as 1x1 stride 1; a fused separable layer is ksize 1.
 * launcher: 0 conv_mfma_kernel, 1 the narrow kernel, 2 the fused separable kernel.  *n_layers: the number of launches (TMAT_E_CAP, with
 * *n_layers set, when it exceeds cap).  The environment switches that choose between kernels (TMAT_FUSED_SEP, TMAT_STEM_FUSED,
 * TMAT_FUSED_POOL) are read as tmat_create reads them.
 * TMAT_E_WEIGHTS, with the rule in tmat_last_error, for a blob tmat_create refuses for its shapes: every filter count has to be a
 * multiple of 16 (at least 16) and, on the down path, 4 times a power of two -- filter_counts (64, 128, 256, 512), (32, 64, 128, 256) and
 * (16, 32, 64, 128) run; (8, 16, 32, 64) or a count of 24 do not.  tmat_create runs the same check before it allocates anything.
 */
int tmat_model_layers(const void *blob, size_t n_bytes, int cap, int *layers, int *n_layers);

/* device memory helpers so a ctypes host can stage inputs in HBM without torch; upload and download are ordered on the handle's
 * stream (a download sees the work queued before it, e.g. tmat_zproj_dev) and return when the copy is done */
int tmat_dev_alloc(tmat_handle h, size_t bytes, void **dev_ptr);
int tmat_dev_free(tmat_handle h, void *dev_ptr);
int tmat_dev_upload(tmat_handle h, void *dev_dst, const void *host_src, size_t bytes);
int tmat_dev_download(tmat_handle h, void *host_dst, const void *dev_src, size_t bytes);

/*
 * Host pixel stages, exposed one by one for stage-wise parity tests (csrc/postproc.cpp): host twins of the device
 * stages.  The batch entry points above run these stages on the GPU (morph_kernels.hip, thin_kernels.hip,
 * finish_kernels.hip); the twins are reached only through these test entry points, TMAT_THIN_DEVICE=0 and images with
 * h^2 + w^2 >= 2^27 -- they are not a fallback for a missing device.
 *   lanczos4: cv2.resize(INTER_LANCZOS4) on u16 (compute_branches.py:312); rescale01: rescale_intensity
 *   (0,1) of an integer image -> f32 (:316); rescale255: rescale_intensity (0,255) in f32 (:419);
 *   filter_mask: transforms.filter_branch_seg_mask (transforms.py:306-361); skeletonize: skimage
 *   skeletonize (transforms.py:331); medial_axis: skimage medial_axis(return_distance=True)
 *   (compute_branches.py:340); permutation: numpy RandomState(seed).permutation(arange(n));
 *   postprocess: compute_branches.py:334-357 for one image.
 */
int tmat_host_lanczos4_u16(const uint16_t *img, int H, int W, int h, int w, uint16_t *out);
int tmat_host_rescale01_u16(const uint16_t *img, size_t n, float *out);
int tmat_host_rescale255_f32(const float *img, size_t n, float *out);
int tmat_host_filter_mask(const uint8_t *mask, int H, int W, int use_median, int remove_isolated, uint8_t *out);
int tmat_host_skeletonize(const uint8_t *mask, int H, int W, uint8_t *out);
int tmat_host_medial_axis(const uint8_t *mask, int H, int W, uint8_t *skel, double *dist);
int tmat_host_permutation(uint32_t seed, int n, uint32_t *out);
int tmat_host_postprocess(const double *pred, int H, int W, int out_h, int out_w, float *field);

/*
 * The one collective of the path (compute_branches.py:585-594 writes its rows from one process; with one process per
 * GPU the rows are gathered first): all-gather of result rows over RCCL.  `rccl_comm` is an ncclComm_t of the caller,
 * `hip_stream` a hipStream_t (NULL = default stream); rows_dev (n_local) and out_dev (world * n_local) are device
 * buffers; every rank passes the same n_local (pad short shards).  Asynchronous on the stream.  The Python host uses
 * torch.distributed's all_gather instead, which is the same RCCL call on torch's communicator.
 */
int tmat_gather_rows(void *rccl_comm, const tmat_row *rows_dev, int n_local, tmat_row *out_dev, void *hip_stream);

/*
 * Z projection of image stacks -- what scripts/compute_zproj.py:73-84 calls through proj_methods
 * (fl_tissue_model_tools/zstacks.py): "fs" proj_focus_stacking (zstacks.py:153-189: cv2.GaussianBlur 5x5 sigma 0, then
 * cv2.Laplacian(CV_64F, ksize 5), per pixel the value of the first slice with the strictly largest |Laplacian|),
 * "min" / "max" (np.min / np.max, :222-249), "avg" (np.mean, :192-204), "med" (np.median, :207-219).
 * stacks (n, Z, H, W) u16 (uint8 stacks are widened by the caller: the arithmetic is the same); out (n, H, W):
 * uint16 for fs / min / max, float64 for avg / med.  tmat_zproj_batch takes host pointers and streams the stacks
 * through the device in chunks; tmat_zproj_dev takes device pointers and is asynchronous on the handle's stream
 * (chain it in front of tmat_analyze_batch_dev).
 */
enum { TMAT_ZPROJ_FS = 0, TMAT_ZPROJ_MIN = 1, TMAT_ZPROJ_MAX = 2, TMAT_ZPROJ_AVG = 3, TMAT_ZPROJ_MED = 4 };
int tmat_zproj_batch(tmat_handle h, const uint16_t *stacks, int n, int Z, int H, int W, int method, void *out);
int tmat_zproj_dev(tmat_handle h, const uint16_t *stacks_dev, int n, int Z, int H, int W, int method, void *out_dev);

/*
 * Arithmetic of the dense convolutions of the UNet (reference: keras Model.predict in float32, models.py:615-622, 644).
 *   TMAT_PRECISION_F32    (default) f32 operands on v_mfma_f32_32x32x2_f32: bit-exact with oracle/unet_exact.c.
 *   TMAT_PRECISION_BF16X3 opt-in split precision: every f32 operand as a bf16 hi + bf16 lo pair, three bf16 MFMAs per
 *                         product (lo*hi + hi*lo + hi*hi) with f32 accumulation; about 2^-16 relative error per product.
 *   TMAT_PRECISION_BF16X6 opt-in: hi + mid + lo (the whole 24-bit mantissa), the six products of order <= 2 (lo*hi, hi*lo,
 *                         mid*mid, mid*hi, hi*mid, hi*hi): 2^-24-level error per product at 3/8 of the f32 path's
 *                         matrix-pipe time.  NOT f32-equivalent at row level: see the measured outcome below.
 *   Neither opt-in mode is bit-exact with the oracle, and NEITHER MEETS the north-star tolerance (branch counts equal, lengths
 *   within 1e-4 relative) at row level on the 256 bench images: measured against the f32 rows (BENCH_r03 "alt" blocks,
 *   profiles/r03_bench.json) bf16x3 flips the branch count of 1 image, bf16x6 of 4 images, and where counts agree the largest
 *   relative length difference is 0.072 in both -- the graph is a discontinuous function of the probability map, so any change of
 *   summation order at the 1e-6 level flips a few rows.  bench.py reports both as a separate "alt" block with "pass": false;
 *   tests/test_gpu_alt_precision.py bounds the probability-map error and records the row flips.  The modes apply to the 3x3 /
 *   sub-pixel / 1x1 convolutions of conv_mfma_kernel; in BF16X3 mode the POINTWISE contraction of the fused separable
 *   convolutions also runs on the bf16 cores (two weight planes; TMAT_SEP_BF16=0 keeps those layers in f32), in BF16X6 mode the
 *   separable layers stay f32 (three planes do not fit the kernel's LDS budget); depthwise taps, stem and final layer are always f32.
 * Takes effect for the calls that follow (all three streams of the handle are drained first).  The environment variable
 * TMAT_PRECISION=f32|bf16x3|bf16x6 selects the mode at tmat_create.
 * A model with narrow layers (tmat_model_layers reports launcher 1 somewhere: filter counts of 16 or 32) is f32 only: an opt-in mode
 * returns TMAT_E_ARG with a message and leaves the handle in f32, through the environment variable it fails tmat_create.
 */
#define TMAT_PRECISION_F32 0
#define TMAT_PRECISION_BF16X3 1
#define TMAT_PRECISION_BF16X6 2
int tmat_set_precision(tmat_handle h, int mode);

/*
 * UNetXceptionPatchSegmentor's optional input normalisation, x = (x - norm_mean) / norm_std in float32 (reference
 * models.py:600-612, 636-637; keys norm_mean / norm_std of the model config), applied on the device in front of
 * predict_img_with_smooth_windowing by every entry point that runs it (tmat_predict_smooth, tmat_segment_batch,
 * tmat_analyze_batch*).  Off by default (the shipped unet_patch_segmentor_1.json has no such keys).
 */
int tmat_set_input_norm(tmat_handle h, int on, double norm_mean, double norm_std);

/*
 * Timing hook for bench.py's roofline line: accumulated HIP-event time (ms) and launch count of
 * the dominant kernel -- tmat::conv_mfma_kernel<128, 128, 4, 2, 3, false>, the 3x3 implicit-GEMM MFMA
 * convolution instantiation that runs 4 of the 8 transposed-conv layers -- since the last reset, measured
 * on the stream it is launched on.  flops = algorithmic FLOPs of those launches.
 */
int tmat_prof_enable(tmat_handle h, int on);
int tmat_prof_read(tmat_handle h, double *ms, int64_t *launches, double *flops, int reset);

/*
 * Test-only (no reference counterpart): fill every scratch workspace the handle owns -- activation buffers, pooled-tile strips,
 * patch_in / patch_out, the scratch block, every per-pass device buffer and pinned mirror -- with `byte_pattern` (0xFF reads as
 * NaN in f32 / f64 and -1 as int).  Constants (weights, window, resize tables) are left alone.  A call that reads a location it
 * has not written itself then fails its bit comparison deterministically (tests/test_gpu_poison.py) instead of depending on
 * what a recycled allocation holds.  Drains the handle's streams before and after.
 */
int tmat_debug_poison(tmat_handle h, int byte_pattern);

/*
 * Test-only (tests/test_gpu_held_memory.py): what the handle retains between calls, in bytes -- exactly the workspaces
 * tmat_debug_poison fills (handle-lifetime buffers, the buffers of the current pass geometry, the side tools' workspaces and the
 * pool of the Z-stack entry points), device and pinned separately.  Constants are not counted.
 */
int tmat_debug_held_bytes(tmat_handle h, size_t *device_bytes, size_t *pinned_bytes);

/*
 * Test-only (tests/test_gpu_morph_stages.py): tmat_filter_mask_batch with its intermediate results.  The same kernels, launches and
 * workspace as tmat_filter_mask_batch; afterwards the stages are copied out of the workspace.  mask (n, h, w) u8.  Outputs, each of
 * which may be null (all of them null is a bad argument, as a null `filtered` is for tmat_filter_mask_batch):
 *   median         (n, h, w) u8    the mask that gets labelled (the 13-tap median of `mask`, or `mask` != 0 with use_median 0)
 *   labels         (n, h, w) i32   smallest flat pixel index (y * w + x, per image) of the pixel's 8-connected component, -1 on background
 *   stats          (n, 4, h, w) i32  area and the perimeter code counts n1, n2, n3 (skimage perimeter, 4-neighbourhood: weights 1,
 *                                  sqrt 2, (1 + sqrt 2) / 2) of each component, stored at its root pixel, 0 everywhere else
 *   skeleton       (n, h, w) u8    the converged Zhang thinning of `median`
 *   filtered       (n, h, w) u8    what tmat_filter_mask_batch returns
 *   thin_launches  (n) i32         thinning launches (4 full iterations each) that removed a pixel of that image
 * Argument checks and the "thinning did not converge" error are tmat_filter_mask_batch's.  A handle from tmat_create_plain is enough.
 */
int tmat_debug_filter_stages(tmat_handle h, const uint8_t *mask, int n, int hh, int ww, int use_median, int remove_isolated, uint8_t *median,
                             int32_t *labels, int32_t *stats, uint8_t *skeleton, uint8_t *filtered, int32_t *thin_launches);

/*
 * Test-only (tests/test_gpu_medial_stages.py): tmat_medial_axis_batch with the intermediate results of its ordered thinning.  The same
 * kernels, launches and workspace as tmat_medial_axis_batch; afterwards the stages are copied out of the workspace.  mask (n, h, w) u8.
 * Outputs, each of which may be null (all of them null is a bad argument):
 *   skel      (n, h, w) u8    what tmat_medial_axis_batch returns
 *   dist      (n, h, w) f64   what tmat_medial_axis_batch returns
 *   keys      (n, h, w) u64   the order key of every pixel: rint(dist^2) << 36 | (9 - foreground count of its 3 x 3 window) << 32 |
 *                             tie[raster-order rank among the image's foreground pixels]; 2^64 - 1 on the background
 *   dep       (n, h, w) u8    the predecessor byte: bit k set when neighbour k (raster order of the 3 x 3 window without its centre,
 *                             NW = bit 0 ... SE = bit 7) lies inside the frame and has a smaller key; 0 on the background
 *   launches  (1) i32         launches of the thinning's round kernel (16 Jacobi rounds each) the call issued, for all n images together
 * Argument checks and the "image too large" refusal are tmat_medial_axis_batch's.  A handle from tmat_create_plain is enough.
 */
int tmat_debug_medial_stages(tmat_handle h, const uint8_t *mask, int n, int hh, int ww, uint8_t *skel, double *dist, uint64_t *keys, uint8_t *dep,
                             int32_t *launches);

/*
 * Region plan of the UNet up path for an (hh, ww) image tiled with `patch`-wide windows (host arithmetic, no GPU and no handle).
 * The smooth blend discards the padding ring, so of every patch it reads the rectangle  patch ∩ interior  only; the tiled entry points
 * compute just that rectangle, grown layer by layer by the taps' reach, in every up-path layer (TMAT_ROI=0 at tmat_create: whole
 * patches, as tmat_unet_predict always does).  Patches with the same rectangle form a class (at most max_classes <= 16; *n_classes = 0
 * reports the fall-back "everything" when there are more).  Within a pass of k images the patches are stored class-major:
 *   position(img, tile) = k * base[c] + img * class_count[c] + tile_rank[tile],  c = tile_class[tile],  base[c] = sum of class_count[< c],
 * tile = the image-major index (orientation-major, then a, then b) of a patch in its image; *tiles_per_img <= tiles_cap of them.
 * channels: n_up + 1 entries, the input channels of up block 0, then the output channels of every up block.
 * Layers l = 0 .. 3 n_up: per up block j the first convolution (3 j; sub-pixel form for j > 0: STORED pixels are enumerated), the residual
 * 1x1 (3 j + 1) and the second convolution (3 j + 2), then the final convolution (stored pixels).
 * rects: [3 n_up + 1][max_classes][4] = y0, x0, rows, columns of what the layer computes for a patch of the class.
 * mac_planned / mac_full: [3 n_up + 1] multiply-accumulates per image, planned and full-frame.
 */
int tmat_roi_plan(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                  int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full);

/*
 * tmat_roi_plan returns the NESTED rectangles: every producer covers its consumer's rounded rectangle plus the taps' reach and rounds
 * its columns again (what TMAT_ROI_TIGHT=0 at tmat_create launches).  tmat_roi_plan_tight returns the TIGHT rectangles of the same
 * classes, patch order and layers (what TMAT_ROI_EXACT=0 at tmat_create launches): every layer computes its own need -- the exact
 * dependency closure of the rectangle the blend reads -- with the columns rounded outwards once by the same rule (first column a
 * multiple of 4; width a multiple of 8, or of 4 below 64 pixels a side, or the whole row), rows exact.  The final convolution's
 * rectangle is the same in both.  A pixel of a tight rectangle outside the need may be computed from operands nobody wrote; nothing
 * the blend reads depends on it.  A tight rectangle lies inside the nested one; mac_planned is that of the rectangles returned.
 * tmat_roi_plan_exact returns the EXACT rectangles, which the tiled entry points launch by default (TMAT_ROI_EXACT, read at tmat_create,
 * default on; it has effect only while TMAT_ROI and TMAT_ROI_TIGHT are on): in every layer but the final convolution the rectangle IS
 * the need, rows and columns, with no rounding -- odd first columns and odd widths are the normal case, and the region form of the
 * convolution kernel takes them (tmat_conv2d_roi; the sub-pixel layers' reads follow the parity of their outputs).  An exact rectangle lies inside the tight one.
 * No export looks at the environment.
 */
int tmat_roi_plan_tight(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                        int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full);
int tmat_roi_plan_exact(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                        int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full);

/*
 * The same plan continued through the down path (classes and patch order are those of tmat_roi_plan): from the rectangle of the
 * bottleneck tensor that up block 0 reads back to the input window.  TMAT_ROI_DOWN at tmat_create is a bit mask of what the tiled entry
 * points run in this form (default 3; 0: the whole down path full-frame; TMAT_ROI=0 switches all region forms off):
 *   bit 0: the unfused level's kernels, the residual 1x1 layers, the stem at the even pixels and the pooling fix-ups;
 *   bit 1: the fused separable layers visit only the 16 x 16 tiles of their rectangles (tmat_roi_sep_tiles; f32 path only, and a
 *          layer whose rectangles are all whole patches keeps the full-frame launch).
 * tmat_create refuses any value but 0 .. 3.
 * up_channels as for tmat_roi_plan; down_channels: n_down + 1 entries (n_down = n_up - 1), the stem's channels, then the output channels
 * of every down block; fused_mask bit b: down block b runs on the fused separable kernel, which computes whole 16 x 16 tiles.
 * Layers l = 0 .. 6 n_down + 3: per down block b (input side patch / 2 >> b) 6 b + 0 .. 3 the first depthwise, first pointwise, second
 * depthwise and second pointwise layer, 6 b + 4 the stride-2 residual 1x1 and 6 b + 5 the max-pool + add (both in OUTPUT pixels); then
 * the stem at its even pixels (side patch / 4), the stem (patch / 2), the input window (patch) and, where the walk starts, the rectangle
 * of the network's output that the blend reads (patch).  The walk follows what that rectangle DEPENDS on, not the rounded rectangles
 * the up-path kernels compute: their extra pixels may see unwritten operands and feed nothing the blend reads.
 * needs: [layers][max_classes][4] = y0, x0, rows, columns the blend depends on; rects: the same rounded outwards to what the layer's
 * kernel computes.  mac_* (pointwise and residual layers) and bytes_* (kernels without matrix work): [layers], per image.
 * free_tile: [n_down], 1 when some class skips a whole tile of a fused level.
 */
int tmat_roi_plan_down(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                       unsigned fused_mask, int max_classes, int *n_classes, int *rects, int *needs, double *mac_planned,
                       double *mac_full, double *bytes_planned, double *bytes_full, int *free_tile);

/*
 * The tiles a fused separable layer of that plan visits in a pass of k images (TMAT_ROI_DOWN bit 1): layer = 6 b + 1 or 6 b + 3 of a
 * level b in fused_mask.  With TW = (patch / 2 >> b) / 16 tiles per row and TPP = TW * TW per patch, tiles[] takes the full-frame ids
 *   position(img, tile) * TPP + ty * TW + tx
 * of the planned tiles: patches in ascending position (class-major, as above), row-major inside the class's rectangle of whole tiles.
 * *n_tiles: their number (<= cap when tiles is given; tiles may be null to ask for the counts only), *n_full = k * tiles_per_img * TPP.
 */
int tmat_roi_sep_tiles(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                       unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles);

/*
 * The constant-ring form of that plan (TMAT_ROI_CONST at tmat_create; the batch pipeline runs it unless the variable is 0,
 * tmat_predict_smooth only when it is 1).  Outside the rectangle of its class that the blend reads, a patch holds one value per image,
 * the pad value.  Per layer and class, all [layers][max_classes][4] = y0, x0, rows, columns:
 *   nonconst:  the pixels whose receptive field, clipped to the patch, reaches the image data.  Outside it the tensor equals, bit for
 *              bit, the tensor of a patch that is the pad value everywhere, at the same position;
 *   live:      what is still computed, need ∩ nonconst; for a tensor that never reaches memory (stored[l] == 0 inside a fused level,
 *              the stem inside the first separable layer) the taps of its consumer's live;
 *   rect_live: live rounded outwards by the rule of rects, inside rects.
 * fill: [layers][max_classes][4 strips][4], the pixels of a stored tensor outside nonconst that a consumer's live reads -- copied from
 * the all-constant patch of the image, which every pass computes beside its patches.  mac_live / bytes_live: mac_planned / bytes_planned
 * of rect_live.  tmat_roi_sep_tiles_live: tmat_roi_sep_tiles for rect_live, a subsequence of that table.
 */
int tmat_roi_plan_const(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                        unsigned fused_mask, int max_classes, int *n_classes, int *nonconst, int *live, int *rect_live, int *fill,
                        int *stored, double *mac_live, double *bytes_live);
int tmat_roi_sep_tiles_live(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                            unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles);

/*
 * The shared-interior form of that plan (TMAT_ROI_SHARE at tmat_create, on top of the constant-ring form: the batch pipeline runs it
 * unless the variable or TMAT_ROI_CONST is 0, tmat_predict_smooth only when it is 1).  The patches of an orientation overlap by half a
 * side, and the down path's tensors hold the same bits in both patches wherever the receptive field crosses neither patch's border.
 * Per layer and class:
 *   inner:  [layers][max_classes][4] = y0, x0, rows, columns: the complement of the ring, the outputs whose receptive field, clipped
 *           to the patch, touches the patch border;
 *   share:  [layers][max_classes][4] = row lo, row hi, column lo, column hi: the positions (per axis) that the next patch on the axis
 *           holds at position - side / 2, computed by itself, whichever patch that is; empty without a successor;
 *   comp:   [layers][max_classes][2][patch] bytes (rows, then columns; the layer's side used): the needed pixels the patch computes
 *           itself, per axis; the 2-D set is the product.
 * fills: [n_fill][7] = layer, class, direction, y0, x0, rows, columns -- the shared pixels of a stored tensor that a consumer taps,
 * copied from the right (0), lower (1) or diagonal (2) neighbour at (y, x - S), (y - S, x), (y - S, x - S), S = side / 2.
 * neighbours: [tiles_per_img][3] image-major tile right of, below, diagonally below a tile, or -1.
 * tmat_roi_sep_tiles_share: the tiles the fused layers still visit, a subsequence of tmat_roi_sep_tiles_live's table in its order.
 */
int tmat_roi_plan_share(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                        unsigned fused_mask, int max_classes, int *n_classes, int *inner, int *share, unsigned char *comp,
                        int fill_cap, int *n_fill, int *fills, int tiles_cap, int *neighbours);
int tmat_roi_sep_tiles_share(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                             unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles);
/*
 * The shared-interior form of the down path's RECTANGLE launches (the unfused 40² level; roi_plan.h:RoiDownPlan::rcomp), in tables of
 * its own: share [6 n_down + 4][max_classes][4] (row lo, row hi, column lo, column hi: the zone of the bottleneck tensor that is copied
 * from the neighbour patches), n_rects [6 n_down + 4][max_classes] and rects [6 n_down + 4][max_classes][4][4] (y0, x0, rows, columns:
 * at most four disjoint rectangles per class, inside rect_live; rect_live itself where the form changes nothing), comp
 * [6 n_down + 4][max_classes][2 axes][patch] bytes (the exact sets before the columns are rounded), fills [n_fill][7] (layer, class,
 * direction, y0, x0, rows, columns), the planned multiply-accumulates and bytes per layer and image, info [3]: some class differs from
 * rect_live, the level that takes the form (-1: none), the longest segment table of a launch.  Host arithmetic, no GPU.
 * The launches take the form where the shared-interior form runs, by the switch TMAT_ROI_SHARE_RECT (read at tmat_create, 0 or 1):
 * unset, the batch pipeline runs it and tmat_predict_smooth does not; 0: nobody; 1: both.
 */
int tmat_roi_plan_share_rect(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                             unsigned fused_mask, int max_classes, int *n_classes, int *share, int *n_rects, int *rects,
                             unsigned char *comp, int fill_cap, int *n_fill, int *fills, double *mac_rect, double *bytes_rect, int *info);
/*
 * The shared-interior form of the FUSED levels' rectangle launches (the stride-2 residual 1x1 and the pooling fix-up of the 160² and 80²
 * levels, the stem at the even pixels; roi_plan.h:RoiDownPlan::fcomp), in tables of its own again: n_rects [6 n_down + 4][max_classes]
 * and rects [6 n_down + 4][max_classes][4][4] (y0, x0, rows, columns: at most four disjoint rectangles per class inside rect_live, what
 * tmat_roi_plan_share_rect gives for every layer the form leaves alone), comp [6 n_down + 4][max_classes][2 axes][patch] bytes (the exact
 * sets in force, every layer, before the columns are rounded), fills [n_fill][7] (layer, class, direction, y0, x0, rows, columns): the
 * copies of a pooled output as halo strips -- only the shared pixels that the next level's exact sets tap --, fill_on [6 n_down + 4]: 1
 * where the strips stand in place of the layer's items of tmat_roi_plan_share, totals [6 n_down + 4][6] per image: planned
 * multiply-accumulates, planned bytes, planned pixels, pixels of rect_live, copied pixels without and with the form, info [3]: some
 * table differs from the older forms', the mask of levels in force, the longest segment table of a launch.  Host arithmetic, no GPU.
 * The launches take the form where the rectangle launches' form of the unfused level runs, by the switch TMAT_ROI_SHARE_FUSED_RECT (read
 * at tmat_create, 0 or 1): unset, the batch pipeline runs it and tmat_predict_smooth does not; 0: nobody; 1: both.
 */
int tmat_roi_plan_share_fused_rect(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                   unsigned fused_mask, int max_classes, int *n_classes, int *n_rects, int *rects, unsigned char *comp,
                                   int fill_cap, int *n_fill, int *fills, int *fill_on, double *totals, int *info);
/*
 * What a down pass of k images launches under one FORM of the down path, composed from the tables above by the one rule the launches
 * themselves read (roi_plan.h:RoiDownForm).  form: 1 the region form (tmat_roi_plan_down), 2 the constant-ring form, 3 the
 * shared-interior form, 4 with the rectangle launches of the unfused level, 5 with those of the fused levels; a form the plan does not
 * have falls back to the highest one below it that it has.  info [4]: the form that runs, the layer whose table the stem at the even
 * pixels launches (6 n_down under form 5, else 4), the longest segment table, and the segment tables of all rectangle launches of the
 * pass added up (with the default kernels, what tmat_debug_down_segs and tmat_debug_down_seg_total report after such a pass).  n_segs [6 n_down + 4] and segs
 * [6 n_down + 4][64][6] (first patch, patches, y0, x0, rows, columns): every layer's segment table in launch order -- the classes in
 * the pass's class-major patch order, up to four rectangles each, then from form 2 upwards one segment of whole patches for the k
 * all-constant patches behind them.  const_fills [n_const][7] (layer, first patch, patches, y0, x0, rows, columns): the strips a
 * stored tensor takes from the constant patches.  copies [n_copy][8] (layer, first patch, patches, direction, y0, x0, rows, columns):
 * the items it then takes from the neighbour patches.  TMAT_E_ARG when a cap is too small.  Host arithmetic, no GPU.
 */
int tmat_roi_down_schedule(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                           unsigned fused_mask, int form, int k, int *info, int *n_segs, int *segs, int const_cap, int *n_const,
                           int *const_fills, int copy_cap, int *n_copy, int *copies);
/*
 * Test-only: the host-side argument checks of the share-fill launcher on a table of n_items items [7] = first patch, patches,
 * direction, y0, x0, rows, columns of a tensor (n_patches, side, side, channels) and a neighbour table [n_patches][3].  Nothing is
 * launched.  TMAT_OK when the launcher would take them; TMAT_E_ARG with the reason in tmat_last_error otherwise.
 */
int tmat_debug_share_fill_check(int n_patches, int side, int channels, const int *neighbours, int n_items, const int *items);
/*
 * The QUADRANT table of a plain fused separable layer (layer = 6 b + 1 of a fused level) for a pass of k images under form 3, 4 or 5
 * (the numbers of tmat_roi_down_schedule; anything else, and every other layer, is refused).  The kernel is organised in 8 x 8
 * quadrants, so a launch may visit any four of them as one packed tile: the table walks the tiles of tmat_roi_sep_tiles_share in
 * their order and lists, per tile in (qy, qx) row-major order, the full-frame id  patch * QW * QW + qy * QW + qx  (QW = side / 8) of
 * every quadrant that holds a pixel of comp (tmat_roi_plan_share); then all four quadrants of every tile of the k all-constant patches
 * behind the pass's patches; then the last id again until the length is a multiple of 4.  counts [4]: the table's length, the ids of
 * the pass's own patches, all ids before the padding, the full-frame tile count of the pass's own patches.  ids (nullable: counts
 * only) takes the table, cap its room.  Host arithmetic, no GPU.
 * The plain fused launches take the table where the shared-interior form or one above it runs, by the switch TMAT_ROI_QUAD (read at
 * tmat_create, 0 or 1): unset, the batch pipeline uses it and tmat_predict_smooth does not; 0: nobody; 1: both.  tmat_debug_sep_tiles
 * then reports the launch's packed tiles (without the constant patches': ceil(counts[1] / 4)) as planned.
 */
int tmat_roi_sep_quads(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                       unsigned fused_mask, int form, int layer, int k, int cap, int *counts, int *ids);
/*
 * Test-only (tests/test_gpu_sep_quads.py): ONE plain fused separable launch in quadrant form on host buffers with the caller's list of
 * n_quads full-frame quadrant ids (any order, any patches, repeats allowed; padded to a multiple of 4 with the last id).  x: (n, hh, ww,
 * cin) float32, or, with the stem's taps [9][cin] and folded batch norm given (all three or none; relu_in 0), the single-channel patches
 * (n, 2 hh, 2 ww) the stem is recomputed from.  dw9: depthwise taps [9][cin]; pw: pointwise weights in the Keras layout (cin, cout).
 * out (n, hh, ww, cout) is caller-filled and changed in place: words of quadrants that are not listed come back as they went in.
 */
int tmat_debug_sepconv_quads(tmat_handle h, const float *x, int n, int hh, int ww, int cin, int relu_in, const float *dw9, const float *pw,
                             int cout, const float *scale, const float *shift, int relu_out, const float *stem_w, const float *stem_scale,
                             const float *stem_shift, const int *quads, int n_quads, float *out);
/*
 * The quadrant table of a POOLED fused separable layer (layer = 6 b + 3 of a fused level): the rule, order, counts and refusals of
 * tmat_roi_sep_quads on that layer's comp.  For every pooled pixel a later launch or copy reads, every quadrant that holds a pixel of
 * its 3 x 3 window inside the patch is listed.  Host arithmetic, no GPU.
 * The pooled fused launches and the pooling fix-up launches behind them take the table where the shared-interior form or one above it
 * runs, by the switch TMAT_ROI_QUAD_POOL (read at tmat_create, 0 or 1; independent of TMAT_ROI_QUAD): unset, the batch pipeline uses it
 * for the levels of ROI_QUAD_POOL_LEVELS (csrc/roi_plan.h) and tmat_predict_smooth does not; 0: nobody; 1: both.  tmat_debug_sep_tiles
 * then reports the launch's packed tiles as planned.
 */
int tmat_roi_sep_quads_pool(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                            unsigned fused_mask, int form, int layer, int k, int cap, int *counts, int *ids);
/*
 * Test-only (tests/test_gpu_sep_quads_pool.py): ONE pooled fused separable launch in quadrant form, and the full-frame quadrant fix-up
 * launch behind it, on host buffers with the caller's list of quadrant ids (as tmat_debug_sepconv_quads).  x: (n, hh, ww, cin); resid
 * and out: (n, hh / 2, ww / 2, cout), cout / 4 a power of two.  out is caller-filled and changed in place: a pooled pixel equals
 * MaxPooling2D(3, 2, "same") + resid where every quadrant its window touches inside the patch is listed; the pooled pixels of a quadrant
 * that is not listed come back as they went in, except its boundary pixels (row 3 and column 3 of its 4 x 4), which the fix-up
 * launch rewrites.
 */
int tmat_debug_sepconv_pool_quads(tmat_handle h, const float *x, int n, int hh, int ww, int cin, int relu_in, const float *dw9, const float *pw,
                                  int cout, const float *scale, const float *shift, int relu_out, const float *resid, const int *quads,
                                  int n_quads, float *out);

/*
 * Test-only (tests/test_gpu_roi_sep.py): the fused separable launches of the handle's last down pass, in launch order -- planned[i]
 * tiles visited of full[i] (equal for a full-frame launch), counted on the host at launch time.  *n: their number (at most cap are
 * written).
 */
int tmat_debug_sep_tiles(tmat_handle h, int cap, int *n, long long *planned, long long *full);
/* Test-only: the longest segment table among the rectangle launches of the last down pass, the constant patches' segment included (0: full-frame). */
int tmat_debug_down_segs(tmat_handle h, int *max_segs);
/* Test-only: the lengths of the segment tables of all rectangle launches of the last down pass added up (the fused levels' form makes no
 * table longer than the longest of the unfused level's form: it shows in this sum). */
int tmat_debug_down_seg_total(tmat_handle h, int *total);

#ifdef __cplusplus
}
#endif
#endif
