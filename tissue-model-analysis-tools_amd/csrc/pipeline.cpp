// Batch drivers of the branching hot path (include/tmat.h): tmat_segment_batch,
// tmat_postprocess_batch, tmat_analyze_batch(_dev) and its masked / tree / extensible / grid forms, tmat_stage_pictures.
//
// Reference control flow: scripts/compute_branches.py:585-594 runs analyze_img one image at a time.
// Here a run is cut into passes of K images (K = max_patches / patches-per-image).  Per pass the GPU
// does Lanczos4 + rescale (preproc_kernels.hip), tile extraction, the UNet over K*200 patches
// (unet_kernels.hip) and the f64 window blend (blend_kernels.hip) on the handle's stream; the
// probability maps come back through pinned memory, and host worker threads run the sequential
// graph stages (postproc.cpp, dmt.cpp, morse.cpp), one image per thread, WHILE the GPU already
// works on the next pass.  Nothing is shared between images, so this is also how the path shards
// across GPUs (one process per GPU, see tmat_amd/distributed.py).
#include "../../include/tmat.h"
#include "overlay.h"
#include "png.h"
#include "tmat_ctx.h"
#include "postproc.h"
#include "morph.h"
#include "host_par.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <chrono>
#include <cstdio>
#include <thread>

namespace tmat {

void launch_lanczos(const uint16_t *img, int n, int H, int W, int h, int w, const int *xi, const float *xc, const int *yi,
                    const float *yc, float *tmp, uint16_t *out, float sat, hipStream_t s);
void launch_rescale01(const uint16_t *x, int n, size_t per, int *mn, int *mx, float *out, hipStream_t s);
void launch_well_zero_f32(float *x, const uint8_t *well, size_t n, hipStream_t s);                             // wellfit_kernels.hip
void launch_well_seg(const double *pred, const uint8_t *well, uint8_t *seg, size_t n, hipStream_t s);

static int round_half_even(double v) { return (int)std::nearbyint(v); }

template <class T> static bool set_ptr(T *&ptr, void *p) { ptr = (T *)p; return p != nullptr; }

// device / pinned buffers for one image geometry, cached on the handle
static int ensure_pass_buffers(Ctx *c, int K, int H, int W, int h, int w, int fh, int fw)
{
    PassBuf &b = c->pass;
    if (b.K >= K && b.H == H && b.W == W && b.h == h && b.w == w && b.fh == fh && b.fw == fw) return TMAT_OK;
    c->free_pass();
    std::vector<int> xi, yi;
    std::vector<float> xc, yc;
    lanczos_axis(W, w, xi, xc);
    lanczos_axis(H, h, yi, yc);
    TMAT_HIP(hipMalloc((void **)&b.xi, xi.size() * 4)); TMAT_HIP(hipMalloc((void **)&b.xc, xc.size() * 4));
    TMAT_HIP(hipMalloc((void **)&b.yi, yi.size() * 4)); TMAT_HIP(hipMalloc((void **)&b.yc, yc.size() * 4));
    TMAT_HIP(hipMemcpy(b.xi, xi.data(), xi.size() * 4, hipMemcpyHostToDevice));
    TMAT_HIP(hipMemcpy(b.xc, xc.data(), xc.size() * 4, hipMemcpyHostToDevice));
    TMAT_HIP(hipMemcpy(b.yi, yi.data(), yi.size() * 4, hipMemcpyHostToDevice));
    TMAT_HIP(hipMemcpy(b.yc, yc.data(), yc.size() * 4, hipMemcpyHostToDevice));
    // every scratch buffer is owned by b.ws: free_pass releases that list, tmat_debug_poison (test-only) fills it between calls
    WsList &ws = b.ws;
    auto dev = [&ws](auto *&ptr, size_t bytes) { return set_ptr(ptr, ws.dev(bytes)); };
    auto pin = [&ws](auto *&ptr, size_t bytes) { return set_ptr(ptr, ws.pinned(bytes)); };
    const size_t px = (size_t)K * h * w, fpx = (size_t)K * fh * fw;
    bool ok = dev(b.tmp, (size_t)K * H * w * sizeof(float)) && dev(b.small, px * sizeof(uint16_t)) && dev(b.x, px * sizeof(float)) &&
              dev(b.mn, (size_t)K * sizeof(int)) && dev(b.mx, (size_t)K * sizeof(int)) && dev(b.morph_ws, morph_workspace_bytes(K, h, w)) &&
              dev(b.finish_ws, finish_workspace_bytes(K, h, w, fh, fw));
    for (int i = 0; i < 2 && ok; i++)
        ok = dev(b.skel[i], px) && pin(b.skel_host[i], px) && dev(b.field[i], fpx * sizeof(float)) && dev(b.f255[i], fpx * sizeof(float)) &&
             pin(b.f255_host[i], fpx * sizeof(float));
    if (ok && thin_dev_supported(h, w)) {
        ok = dev(b.thin_ws, thin_workspace_bytes(K, h, w)) && dev(b.tie, px * sizeof(uint32_t));
        for (int i = 0; i < 2 && ok; i++)
            ok = dev(b.nfg[i], (size_t)K * sizeof(int)) && pin(b.nfg_host[i], (size_t)K * sizeof(int)) && pin(b.tie_host[i], px * sizeof(uint32_t));
    }
    if (ok && fh >= 2 && fw >= 2) {
        const size_t nE = (size_t)K * dmt_edge_count(fh, fw);
        ok = dev(b.dmt_ws, dmt_workspace_bytes(K, fh, fw));
        for (int i = 0; i < 2 && ok; i++)
            ok = dev(b.dmt_ids[i], nE * sizeof(int32_t)) && pin(b.dmt_ids_host[i], nE * sizeof(int32_t)) && dev(b.dmt_m[i], (size_t)K * sizeof(int)) &&
                 pin(b.dmt_m_host[i], (size_t)K * sizeof(int));
        if (ok && c->dmt_device && c->dmt_sweep_device) {
            ok = dev(b.dmt_sweep_ws, dmt_sweep_workspace_bytes(K, fh, fw));
            for (int i = 0; i < 2 && ok; i++)
                ok = dev(b.dmt_kind[i], nE) && pin(b.dmt_kind_host[i], nE) && dev(b.dmt_pers[i], nE * sizeof(float)) && pin(b.dmt_pers_host[i], nE * sizeof(float));
        }
    }
    b.fh = fh; b.fw = fw;
    for (int i = 0; i < 2 && ok; i++)
        ok = dev(b.pred[i], px * sizeof(double)) && pin(b.pred_host[i], px * sizeof(double)) && dev(b.filt[i], px) && dev(b.dist[i], px * sizeof(double)) &&
             pin(b.filt_host[i], px) && pin(b.dist_host[i], px * sizeof(double)) && pin(b.conv_host[i], (size_t)K * sizeof(int)) &&
             hip_ok(hipEventCreateWithFlags(&b.done[i], hipEventDisableTiming), "hipEventCreate");
    if (!ok) return TMAT_E_HIP;
    b.K = K; b.H = H; b.W = W; b.h = h; b.w = w;
    return TMAT_OK;
}

// the decision table of the ordered thinning, uploaded once per handle
static int ensure_ma_table(Ctx *c)
{
    if (c->ma_table) return TMAT_OK;
    uint32_t bits[16];
    medial_table_bits(bits);
    TMAT_HIP(hipMalloc((void **)&c->ma_table, sizeof(bits)));
    TMAT_HIP(hipMemcpy(c->ma_table, bits, sizeof(bits), hipMemcpyHostToDevice));
    return TMAT_OK;
}
static bool thin_on_device(const Ctx *c) { return c->thin_device && c->pass.thin_ws != nullptr; }

// GPU part of one pass: imgs_dev (k, H, W) u16 -> pred (k, h, w) f64 in b.pred[slot], copied to pinned host
static int enqueue_segment(Ctx *c, const uint16_t *imgs_dev, int k, int slot)
{
    PassBuf &b = c->pass;
    launch_lanczos(imgs_dev, k, b.H, b.W, b.h, b.w, b.xi, b.xc, b.yi, b.yc, b.tmp, b.small, c->input_sat, c->stream);
    launch_rescale01(b.small, k, (size_t)b.h * b.w, b.mn, b.mx, b.x, c->stream);
    int rc = predict_smooth_dev(c, b.x, k, b.h, b.w, b.pred[slot]);
    if (rc) return rc;
    TMAT_HIP(hipMemcpyAsync(b.pred_host[slot], b.pred[slot], (size_t)k * b.h * b.w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TMAT_HIP(hipEventRecord(b.done[slot], c->stream));
    return TMAT_OK;
}

// Two-stream form used by tmat_analyze_batch*: the memory-bound front half of pass p+1 (Lanczos, rescale, tile
// gather, UNet down path) runs on stream2 while the MFMA-bound back half of pass p (UNet up path, final conv, blend,
// D2H) runs on the main stream.
static bool use_one_stream()
{
    static const bool one = [] { const char *e = getenv("TMAT_STREAMS"); return !(e && atoi(e) == 2); }();
    return one;
}
// the tail of a pass (blend, mask filter, EDT, copies) on the second stream: see enqueue_back
static bool tail_on_side_stream()
{
    static const bool side = [] { const char *e = getenv("TMAT_TAIL_STREAM"); return !(e && atoi(e) == 0); }() && use_one_stream();
    return side;
}
// The front end of a pass (Lanczos, rescale, tile gather: ~2 ms of memory-bound kernels) runs on the SECOND stream, ahead of time: the
// one of pass p + 2 is queued when pass p's tail has finished, beside pass p + 1's network, into the input buffer pass p has released
// (patch_in / patch_in2 alternate), so that on the main stream one pass's network follows the other's directly (TMAT_PRE_STREAM=0 keeps
// it on the main stream in front of its down path).  An image that needs more patches than the activation workspace holds takes the
// old route: everything on the main stream, one input buffer.
static bool pre_on_side_stream(const Ctx *c, const TileGeom &g) { return c->pre_side && tail_on_side_stream() && g.tiles_per_img <= c->max_patches && c->patch_in2; }
static float *patch_in_of(Ctx *c, int slot, const TileGeom &g) { return pre_on_side_stream(c, g) && (slot & 1) ? c->patch_in2 : c->patch_in; }
// bg_keep (nullable, the "with tree" form only): the pass's down-sampled images are copied there, b.small itself is rewritten by the next pass
// well (nullable, the masked form only): the pass's (k, h, w) well masks on the device -- img * well_mask (compute_branches.py:328) in front
// of the normalisation, as predict() sees it; the pad minimum is taken after it
// orig_pic (nullable, stage pictures only): (k, h, w) u8 on the device for original_image.png (compute_branches.py:315) -- rendered HERE,
// behind the rescale on its stream: b.small, b.mn and b.mx are single buffers that the front end of the pass after next rewrites
static int enqueue_pre(Ctx *c, const uint16_t *imgs_dev, int k, int slot, const TileGeom &g, uint16_t *bg_keep = nullptr, const uint8_t *well = nullptr,
                       uint8_t *orig_pic = nullptr)
{
    PassBuf &b = c->pass;
    const bool oversize = g.tiles_per_img > c->max_patches;
    const bool side = pre_on_side_stream(c, g);
    hipStream_t s = side ? c->stream2 : (use_one_stream() || oversize) ? c->stream : c->stream2;
    // the down path of the pass before last read this buffer (long finished: its whole pass has ended; stated for the record)
    if (side && c->down_pending[slot]) TMAT_HIP(hipStreamWaitEvent(s, c->ev_down[slot], 0));
    launch_lanczos(imgs_dev, k, b.H, b.W, b.h, b.w, b.xi, b.xc, b.yi, b.yc, b.tmp, b.small, c->input_sat, s);
    if (bg_keep) TMAT_HIP(hipMemcpyAsync(bg_keep, b.small, (size_t)k * b.h * b.w * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
    launch_rescale01(b.small, k, (size_t)b.h * b.w, b.mn, b.mx, b.x, s);
    if (orig_pic && vis_picture_u16_dev(b.small, k, (size_t)b.h * b.w, b.mn, b.mx, orig_pic, s)) { set_error("analyze (pictures): launch failed"); return TMAT_E_HIP; }
    if (well) launch_well_zero_f32(b.x, well, (size_t)k * b.h * b.w, s);
    if (c->norm_on) launch_norm_f32(b.x, (size_t)k * b.h * b.w, c->norm_mean, c->norm_std, s);      // models.py:636-637
    float *mn = (float *)c->scratch, *mx = mn + k;
    launch_minmax_f32(b.x, k, (size_t)b.h * b.w, mn, mx, s);
    launch_extract_tiles(b.x, mn, k, g, patch_in_of(c, slot, g), s);
    // the pad values until the pass's down path runs (the constant-ring form): mn is rewritten by the front end of the pass after next
    if (c->roi_const != 0 && k <= c->const_cap) TMAT_HIP(hipMemcpyAsync(c->padval[slot], mn, (size_t)k * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (side) TMAT_HIP(hipEventRecord(c->ev_pre[slot], s));
    return TMAT_OK;
}
static int enqueue_down(Ctx *c, int k, int slot, const TileGeom &g)
{
    // Default: the network on the main stream.  TMAT_STREAMS=2 puts the front end and the down path on the second stream; measured +1.8 %
    // images/s, but every kernel of the MFMA half then shares the CUs with a memory-bound one and its own duration
    // (the roofline measurement) stretches by 20 %, so the overlap is opt-in.
    // an image that needs more patches than the activation workspace holds: the whole network runs here, chunk by
    // chunk, on the main stream (enqueue_back then only blends)
    const bool oversize = g.tiles_per_img > c->max_patches;
    hipStream_t s = (use_one_stream() || oversize) ? c->stream : c->stream2;
    if (pre_on_side_stream(c, g)) TMAT_HIP(hipStreamWaitEvent(s, c->ev_pre[slot], 0));
    // oversize: the whole network runs HERE and writes the single patch_out, which the blend of the previous pass may still be
    // reading on the second stream (enqueue_back's own wait on ev_blend comes too late: it is issued after this forward)
    if (oversize && tail_on_side_stream() && c->blend_pending[slot ^ 1]) TMAT_HIP(hipStreamWaitEvent(s, c->ev_blend[slot ^ 1], 0));
    float *pin = patch_in_of(c, slot, g);
    const RoiPlan *plan = roi_find(c, g);
    int rc = oversize ? unet_forward_dev(c, pin, k * g.tiles_per_img, c->patch_out, s)
                      : unet_down_dev(c, pin, k * g.tiles_per_img, c->dout[slot], s, plan, c->padval[slot],
                                      roi_down_resolve(c, plan, k, c->padval[slot] != nullptr, true), roi_quad_on(c, true), roi_quad_pool_on(c, true));
    if (rc) return rc;
    TMAT_HIP(hipEventRecord(c->ev_down[slot], s));
    c->down_pending[slot] = true;
    return TMAT_OK;
}
// well / seg (nullable, the masked form only): the mask filter starts from (pred > 0.5) & well (compute_branches.py:334), formed in seg;
// b.pred stays unmasked -- the centre-line weighting reads it (:344)
static int enqueue_back(Ctx *c, int k, int slot, const TileGeom &g, const uint8_t *well = nullptr, uint8_t *seg = nullptr)
{
    PassBuf &b = c->pass;
    hipStream_t s = c->stream;
    TMAT_HIP(hipStreamWaitEvent(s, c->ev_down[slot], 0));
    // The tail of a pass -- blend, mask filter, EDT, the copies: ~8 ms of small kernels (83 Zhang launches among them) that leave most
    // of the chip idle -- runs on the second stream, so that the next pass's network follows this pass's network directly on the main
    // stream: 31.28 -> 31.58 images/s (TMAT_TAIL_STREAM=0 keeps everything on the main stream).  patch_out is single: the next up path
    // waits for this pass's blend.  (Round 2 tried the same with a low-priority stream and saw nothing; the second stream has normal priority.)
    const bool tail_side = tail_on_side_stream();
    if (tail_side && c->blend_pending[slot ^ 1]) TMAT_HIP(hipStreamWaitEvent(s, c->ev_blend[slot ^ 1], 0));
    int rc = g.tiles_per_img > c->max_patches ? TMAT_OK : unet_up_dev(c, c->dout[slot], k * g.tiles_per_img, c->patch_out, s, roi_find(c, g));
    if (rc) return rc;
    if (tail_side) {
        TMAT_HIP(hipEventRecord(c->ev_up[slot], s));
        s = c->stream2;
        TMAT_HIP(hipStreamWaitEvent(s, c->ev_up[slot], 0));
    }
    launch_blend(c->patch_out, c->win1d, k, g, b.pred[slot], s);
    if (tail_side) { TMAT_HIP(hipEventRecord(c->ev_blend[slot], s)); c->blend_pending[slot] = true; }
    // binary morphology on the GPU: threshold, median, labelling, perimeter, thinning, fork test, EDT (remove_isolated=True
    // is filter_branch_seg_mask's default, compute_branches.py:337)
    const size_t npx = (size_t)k * b.h * b.w;
    if (well) {
        launch_well_seg(b.pred[slot], well, seg, npx, s);
        rc = filter_mask_dev(nullptr, seg, k, b.h, b.w, 1, 1, b.morph_ws, b.filt[slot], b.dist[slot], s);
    } else {
        rc = filter_edt_dev(b.pred[slot], k, b.h, b.w, 1, b.morph_ws, b.filt[slot], b.dist[slot], s);
    }
    if (rc) return TMAT_E_HIP;
    if (thin_on_device(c)) {
        // the ordered thinning runs on the device too: the host only needs the foreground counts (for the permutations)
        if (thin_count_dev(b.filt[slot], k, b.h, b.w, b.nfg[slot], s)) return TMAT_E_HIP;
        TMAT_HIP(hipMemcpyAsync(b.nfg_host[slot], b.nfg[slot], k * sizeof(int), hipMemcpyDeviceToHost, s));
    } else {
        TMAT_HIP(hipMemcpyAsync(b.filt_host[slot], b.filt[slot], npx, hipMemcpyDeviceToHost, s));
        TMAT_HIP(hipMemcpyAsync(b.dist_host[slot], b.dist[slot], npx * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    TMAT_HIP(hipMemcpyAsync(b.conv_host[slot], morph_done_flags(b.morph_ws, k, b.h, b.w), k * sizeof(int), hipMemcpyDeviceToHost, s));
    TMAT_HIP(hipEventRecord(b.done[slot], s));
    return TMAT_OK;
}

struct GraphParams {
    int fh, fw;
    float t1, t2;
    int smooth, min_len, max_len, remove_isolated;
};

// host part for one image: pred (h, w) f64 -> row
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static bool trace_on() { static int t = -1; if (t < 0) { const char *e = getenv("TMAT_TRACE"); t = e && atoi(e) > 0; } return t; }

// n_workers / parallel_images: host_par.h (shared with the Z-stack batch pipeline)

// Host coordinator of one pass (runs in its own thread while the GPU works on the next pass):
//   1. ordered medial-axis thinning per image (sequential by construction)            host threads
//   2. EDT(~skeleton), weighting, resize, rescale on the third stream                 GPU (finish_kernels.hip)
//   3. DMT sweeps + collect + MorseGraph statistics per image                         host threads
struct PassJob {
    std::thread th;
    std::atomic<int> rc{0};
    void join() { if (th.joinable()) th.join(); }
};

// The "with tree" form of a call (tmat_analyze_batch_tree*): per image the branch geometry instead of the statistics alone, and per pass
// one rasteriser launch set on the third stream over the pass's down-sampled images (kept in bg_all), overlays copied to the caller.
struct TreeJob {
    Canvas cv;
    double sf;                      // compute_branches.py:437: original_image.shape[1] / img_dsamp_res[1]
    uint8_t *rgb_out; double *bars_out; int cap_b; int *n_bars;     // caller's, whole call
    uint16_t *bg_all;               // (n, h, w) u16 on the device, written by enqueue_pre
    OverlaySeg *dseg; size_t seg_cap; float *dmm; int *doff; uint8_t *drgb;
    // the grid form only (tmat_analyze_batch_grid*): rgb_out may then be null, and the pictures may leave as PNG files, encoded on the
    // third stream from the rasters in HBM (png_kernels.hip) -- the overlays from drgb, the barcodes from dbar (overlay_kernels.hip)
    uint8_t *tree_png; size_t tree_png_cap; size_t *tree_png_sizes; PngShape pg_tree;
    uint8_t *barcode_png; size_t barcode_png_cap; size_t *barcode_png_sizes; PngShape pg_bar;
    int S; BarRect *drect; int *drect_off; uint8_t *dbar;
    uint8_t *png_filt, *png_slots, *png_files; uint32_t *png_meta, *png_dsz; int png_mode;
};

// The pairs of a call: tmat_analyze_batch_grid* sweeps T (graph_thresh_1, graph_thresh_2) pairs from ONE pass of the network; every
// other entry is the grid of its one pair.  Per-pair outputs carry a leading T axis: item (t, i) of a call of n images sits at t n + i.
struct GridJob { int T; const float *thresh; int n; };

// images of one encoder launch set: <= 128 MiB of filtered stream, as png_encode_ctx
static int png_chunk(const PngShape &g, int k) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)k, ((size_t)128 << 20) / g.raw)); }
static size_t png_fcap(const PngShape &g) { return (g.bound + 15) & ~(size_t)15; }

// k pictures of shape g in HBM -> k files at out + i cap_each on the host, on stream s with the job's encoder scratch (two
// synchronisations per launch set: the sizes come back first, then exactly the files' bytes)
static int png_encode_job(const TreeJob &tj, const uint8_t *pics_dev, int k, const PngShape &g, uint8_t *out, size_t cap_each, size_t *sizes, hipStream_t s)
{
    const size_t pic_bytes = (size_t)g.H * g.rb, fcap = png_fcap(g);
    const int Kp = png_chunk(g, k);
    std::vector<uint32_t> hsz(Kp);
    for (int i0 = 0; i0 < k; i0 += Kp) {
        const int kk = std::min(Kp, k - i0);
        if (png_encode_launch(pics_dev + (size_t)i0 * pic_bytes, kk, g, tj.png_mode, tj.png_filt, tj.png_slots, tj.png_meta, tj.png_files, fcap, tj.png_dsz, s)) {
            set_error("analyze (grid): png encoder launch failed");
            return TMAT_E_HIP;
        }
        if (hipMemcpyAsync(hsz.data(), tj.png_dsz, (size_t)kk * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return TMAT_E_HIP;
        for (int i = 0; i < kk; i++) {
            if (hsz[i] < PNG_HEAD + PNG_TAIL || hsz[i] > g.bound) { set_error("png encoder: a file left its bound"); return TMAT_E_HIP; }
            if (hipMemcpyAsync(out + (size_t)(i0 + i) * cap_each, tj.png_files + (size_t)i * fcap, hsz[i], hipMemcpyDeviceToHost, s) != hipSuccess) return TMAT_E_HIP;
            sizes[i0 + i] = hsz[i];
        }
        if (hipStreamSynchronize(s) != hipSuccess) return TMAT_E_HIP;
    }
    return TMAT_OK;
}

// The stage pictures of a call (tmat_analyze_batch_ex with stage_out): save_vis of the four arrays the reference dumps, rendered from
// the pass's own buffers (vis_kernels.hip) and copied to the caller's (n, 4, h, w) array per pass.
struct StageJob {
    uint8_t *out;                   // caller's, whole call
    uint8_t *orig_all;              // (n, h, w) u8 on the device, written by enqueue_pre
    uint8_t *pics;                  // (3, K, h, w) u8 on the device: prediction, mask, weighted of one pass
    void *mm;                       // vis_scratch_bytes(K)
    int K;
};

// pruning (nullable, the masked form only): the pass's (k, fh, fw) u8 pruning masks on the host, MorseGraph's pruning_mask per image
// rows: the CALL's rows, (T, n); the pass's images are first_img .. first_img + k of every pair
static void run_pass_host(Ctx *c, int slot, int k, const GraphParams gp, const GridJob gj, tmat_row *rows, PassJob *job, const TreeJob *tree = nullptr,
                          int first_img = 0, const uint8_t *pruning = nullptr, const StageJob *stage = nullptr)
{
    PassBuf &b = c->pass;
    const int h = b.h, w = b.w;
    const size_t per = (size_t)h * w, fper = (size_t)gp.fh * gp.fw;
    const double t0 = now_s();
    double t_perm = t0;
    hipSetDevice(c->device);
    hipStream_t s = c->stream3;
    bool ok = true;
    if (thin_on_device(c)) {
        // host part of the medial axis: the RandomState(0) tie-break permutation of every image's foreground count
        parallel_images(k, [&](int i) {
            std::vector<uint32_t> perm;
            legacy_permutation(0, (size_t)b.nfg_host[slot][i], perm);
            std::memcpy(b.tie_host[slot] + i * per, perm.data(), perm.size() * sizeof(uint32_t));
        });
        t_perm = now_s();
        for (int i = 0; i < k && ok; i++)
            ok = hipMemcpyAsync(b.tie + i * per, b.tie_host[slot] + i * per, (size_t)b.nfg_host[slot][i] * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess;
        ok = ok && thin_dev(b.filt[slot], b.dist[slot], b.tie, b.nfg[slot], k, h, w, b.thin_ws, c->ma_table, b.skel[slot], s) == 0;
    } else {
        parallel_images(k, [&](int i) { medial_axis_thin(b.filt_host[slot] + i * per, b.dist_host[slot] + i * per, h, w, b.skel_host[slot] + i * per); });
        ok = hipMemcpyAsync(b.skel[slot], b.skel_host[slot], k * per, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    const double t1 = now_s();
    ok = ok && finish_dev(b.pred[slot], b.dist[slot], b.skel[slot], k, h, w, gp.fh, gp.fw, b.finish_ws, b.field[slot], b.f255[slot], s) == 0;
    ok = ok && hipMemcpyAsync(b.f255_host[slot], b.f255[slot], k * fper * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess;
    // DMT front end on the device: edge keys + lower-star sort from the field in HBM; the sorted edge ids come back
    const bool dmt_dev = c->dmt_device && b.dmt_ws && gp.fh >= 2 && gp.fw >= 2;
    const size_t nE = dmt_dev ? dmt_edge_count(gp.fh, gp.fw) : 0;
    if (dmt_dev) {
        ok = ok && dmt_sorted_edges_dev(b.f255[slot], k, gp.fh, gp.fw, b.dmt_ws, b.dmt_ids[slot], b.dmt_m[slot], s) == 0;
        ok = ok && hipMemcpyAsync(b.dmt_ids_host[slot], b.dmt_ids[slot], k * nE * sizeof(int32_t), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = ok && hipMemcpyAsync(b.dmt_m_host[slot], b.dmt_m[slot], k * sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    // ... and the two persistence sweeps (one workgroup per image, one launch): pairing kind + persistence per sorted edge
    const bool sweep_dev = dmt_dev && b.dmt_sweep_ws;
    if (sweep_dev) {
        ok = ok && dmt_sweeps_dev(b.f255[slot], b.dmt_ids[slot], b.dmt_m[slot], k, gp.fh, gp.fw, b.dmt_sweep_ws, b.dmt_kind[slot], b.dmt_pers[slot], s) == 0;
        ok = ok && hipMemcpyAsync(b.dmt_kind_host[slot], b.dmt_kind[slot], k * nE, hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = ok && hipMemcpyAsync(b.dmt_pers_host[slot], b.dmt_pers[slot], k * nE * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (stage && ok) {
        // b.pred / b.filt of this slot stay as they are until this job ends; wt and its extrema lie in finish_ws, which only this job uses
        // (one host job runs at a time); the original picture was finished before the pass's `done` event
        const double *wt, *wlo, *whi;
        finish_weighted_view(b.finish_ws, k, h, w, &wt, &wlo, &whi);
        double *lo = vis_scratch_lo(stage->mm, k), *hi = lo + k;
        uint8_t *pic[3] = {stage->pics, stage->pics + (size_t)stage->K * per, stage->pics + 2 * (size_t)stage->K * per};
        ok = vis_minmax_dev(b.pred[slot], TMAT_PIC_F64, k, per, stage->mm, s) == 0 && vis_picture_dev(b.pred[slot], TMAT_PIC_F64, k, per, lo, hi, pic[0], s) == 0 &&
             vis_minmax_dev(b.filt[slot], TMAT_PIC_U8, k, per, stage->mm, s) == 0 && vis_picture_dev(b.filt[slot], TMAT_PIC_U8, k, per, lo, hi, pic[1], s) == 0 &&
             vis_picture_dev(wt, TMAT_PIC_F64, k, per, wlo, whi, pic[2], s) == 0;
        for (int i = 0; i < k && ok; i++) {
            uint8_t *dst = stage->out + (size_t)(first_img + i) * 4 * per;
            ok = hipMemcpyAsync(dst + TMAT_STAGE_ORIGINAL * per, stage->orig_all + (size_t)(first_img + i) * per, per, hipMemcpyDeviceToHost, s) == hipSuccess &&
                 hipMemcpyAsync(dst + TMAT_STAGE_PREDICTION * per, pic[0] + i * per, per, hipMemcpyDeviceToHost, s) == hipSuccess &&
                 hipMemcpyAsync(dst + TMAT_STAGE_MASK * per, pic[1] + i * per, per, hipMemcpyDeviceToHost, s) == hipSuccess &&
                 hipMemcpyAsync(dst + TMAT_STAGE_WEIGHTED * per, pic[2] + i * per, per, hipMemcpyDeviceToHost, s) == hipSuccess;
        }
    }
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { job->rc = TMAT_E_HIP; return; }
    const double t2 = now_s();
    // the graph stage over (pair, image): every item reads the pass's ONE set of mirrors (field, sorted edge ids, pairing kinds and
    // persistences: none depends on the thresholds) and runs `collect` (dmt.cpp) with its pair's thresholds
    const int T = gj.T;
    const size_t n_all = (size_t)gj.n;
    std::vector<std::vector<double>> tsegs(tree ? (size_t)T * k : 0);
    std::vector<std::vector<int32_t>> tbranch(tree ? (size_t)T * k : 0);
    parallel_images(T * k, [&](int item) {
        const int t = item / k, i = item % k;
        const size_t at = (size_t)t * n_all + first_img + i;        // (t, image of the call)
        tmat_row &row = rows[at];
        const int cap_v = (int)fper + 4, cap_e = 3 * (int)fper + 4;
        std::vector<int32_t> V((size_t)cap_v * 2), E((size_t)cap_e * 2);
        int nv = 0, ne = 0;
        int rc = dmt_graph_host_sorted(b.f255_host[slot] + i * fper, gp.fh, gp.fw, gj.thresh[2 * t], gj.thresh[2 * t + 1],
                                       dmt_dev ? b.dmt_ids_host[slot] + i * nE : nullptr,
                                       dmt_dev ? b.dmt_m_host[slot][i] : 0, V.data(), cap_v, E.data(), cap_e, &nv, &ne,
                                       sweep_dev ? b.dmt_kind_host[slot] + i * nE : nullptr, sweep_dev ? b.dmt_pers_host[slot] + i * nE : nullptr);
        if (!rc && !tree)
            rc = tmat_morse_stats(V.data(), nv, E.data(), ne, gp.fh, gp.fw, gp.smooth, gp.min_len, gp.max_len, gp.remove_isolated,
                                  pruning ? pruning + i * fper : nullptr, &row.count, &row.total_px, &row.avg_px, nullptr, 0);
        if (!rc && tree)
            rc = morse_tree_item(V.data(), nv, E.data(), ne, gp.fh, gp.fw, gp.smooth, gp.min_len, gp.max_len, gp.remove_isolated,
                                 pruning ? pruning + i * fper : nullptr, tree->sf, &row.count, &row.total_px, &row.avg_px, tsegs[item], tbranch[item],
                                 tree->bars_out + at * tree->cap_b * 2, tree->cap_b, tree->n_bars + at);
        if (rc) job->rc = rc;
    });
    if (tree && !job->rc) {
        // the pictures, pair by pair on the third stream: the pass's K canvases (drgb, dbar) and its segment / rectangle tables are reused
        // by every pair, so each pair ends with a synchronisation (which also releases its host tables)
        const bool render = tree->rgb_out || tree->tree_png;
        const size_t cper = (size_t)tree->cv.vh * tree->cv.vw * 3;
        const uint16_t *bg = tree->bg_all + (size_t)first_img * per;
        int rc = TMAT_OK;
        if (render && overlay_minmax_dev(bg, 0, k, h, w, tree->dmm, s)) rc = TMAT_E_HIP;        // the backgrounds' extrema: once per pass
        for (int t = 0; t < T && !rc; t++) {
            const size_t at = (size_t)t * n_all + first_img;
            std::vector<OverlaySeg> ss;
            std::vector<int> off(k + 1, 0), roff(k + 1, 0);
            std::vector<BarRect> rects;
            if (render) {
                rc = overlay_pair_dev(bg, 0, k, h, w, tree->cv, &tsegs[(size_t)t * k], &tbranch[(size_t)t * k],
                                      OverlayWs{tree->dseg, tree->seg_cap, tree->dmm, tree->doff, tree->drgb}, ss, off,
                                      tree->rgb_out ? tree->rgb_out + at * cper : nullptr, "analyze (tree)", s);
                if (!rc && tree->tree_png)
                    rc = png_encode_job(*tree, tree->drgb, k, tree->pg_tree, tree->tree_png + at * tree->tree_png_cap, tree->tree_png_cap, tree->tree_png_sizes + at, s);
            }
            if (!rc && tree->barcode_png) {
                for (int i = 0; i < k; i++) {
                    barcode_rects(tree->bars_out + (at + i) * tree->cap_b * 2, tree->n_bars[at + i], tree->S, rects);
                    roff[i + 1] = (int)rects.size();
                }
                if ((!rects.empty() && hipMemcpyAsync(tree->drect, rects.data(), rects.size() * sizeof(BarRect), hipMemcpyHostToDevice, s) != hipSuccess) ||
                    hipMemcpyAsync(tree->drect_off, roff.data(), (size_t)(k + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) rc = TMAT_E_HIP;
                if (!rc && barcode_render_dev(tree->drect, tree->drect_off, k, tree->S, tree->dbar, s)) { set_error("analyze (grid): barcode launch failed"); rc = TMAT_E_HIP; }
                if (!rc)
                    rc = png_encode_job(*tree, tree->dbar, k, tree->pg_bar, tree->barcode_png + at * tree->barcode_png_cap, tree->barcode_png_cap,
                                        tree->barcode_png_sizes + at, s);
            }
            if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = TMAT_E_HIP;       // ss / off / rects are released here
        }
        if (rc) job->rc = rc;
    }
    if (trace_on())
        fprintf(stderr, "[tmat] host pass (%d images): ordered thinning %.1f ms (host permutations %.1f, the rest = its launches and convergence polls on the low-priority stream), finish + DMT on the GPU %.1f ms, collect + Morse %.1f ms\n", k,
                (t1 - t0) * 1e3, (t_perm - t0) * 1e3, (t2 - t1) * 1e3, (now_s() - t2) * 1e3);
}

// One call of the 2-D batch analysis family: what any tmat_analyze_batch* entry point can ask for.  Every entry fills one and hands it to
// analyze_entry (below), which checks it, uploads host images and runs analyze_dev.
struct AnalyzeCall {
    const char *name;               // the entry point the caller called: heads the error messages
    const uint16_t *imgs; bool host;        // (n, H, W) u16, on the host (analyze_entry uploads them) or on the device
    int n, H, W;
    double ds_ratio; int ds_width;
    GraphParams gp;                 // fh / fw are filled by analyze_dev; t1 / t2 are not read in the grid form
    int64_t first_index;
    tmat_row *rows;
    // the "with tree" form: rgb_out may be null in the grid form when the pictures leave as PNG files
    bool tree; int vis_width; uint8_t *rgb_out; double *bars_out; int cap_b; int *n_bars;
    // the masked form, both on the HOST and either may be null: well (n, h, w) u8 multiplies the network input and the thresholded mask,
    // pruning (n, fh, fw) u8 is MorseGraph's pruning mask
    const uint8_t *well, *pruning;
    uint8_t *stage_out;             // nullable: (n, 4, h, w) u8 stage pictures
    // nullable, tmat_analyze_batch_grid* only: the pairs of the call instead of gp.t1 / gp.t2 -- rows and the tree outputs gain a leading
    // n_thresh axis, and the pictures may leave as PNG files
    const tmat_grid_opts *grid;
};

// The canvas of a tree request and the file shapes of the grid form's PNG outputs: checked (capacities included) before anything is
// allocated or queued
static int tree_shapes(const AnalyzeCall &call, int h, int w, TreeJob &tj)
{
    const std::string name = call.name;
    const tmat_grid_opts *grid = call.grid;
    if (!canvas_of(h, w, call.vis_width, tj.cv)) { set_error("analyze (tree): empty canvas"); return TMAT_E_ARG; }
    if (grid && grid->tree_png) {
        if (!png_shape(tj.cv.vh, tj.cv.vw, 3, tj.pg_tree)) { set_error(name + ": canvas too large for one PNG file"); return TMAT_E_ARG; }
        if (grid->tree_png_cap < tj.pg_tree.bound) { set_error(name + ": tree_png_cap is below tmat_png_bound"); return TMAT_E_CAP; }
        tj.tree_png = grid->tree_png; tj.tree_png_cap = grid->tree_png_cap; tj.tree_png_sizes = grid->tree_png_sizes;
    }
    if (grid && grid->barcode_png) {
        tj.S = barcode_side(call.vis_width);
        if (!png_shape(tj.S, tj.S, 3, tj.pg_bar)) { set_error(name + ": empty barcode canvas, or one too large for a PNG file"); return TMAT_E_ARG; }
        if (grid->barcode_png_cap < tj.pg_bar.bound) { set_error(name + ": barcode_png_cap is below tmat_png_bound"); return TMAT_E_CAP; }
        tj.barcode_png = grid->barcode_png; tj.barcode_png_cap = grid->barcode_png_cap; tj.barcode_png_sizes = grid->barcode_png_sizes;
    }
    return TMAT_OK;
}

// scratch of the "with tree" form: the handle's tool workspaces, sized before any pass is in flight (tj holds tree_shapes' results)
static int tree_setup(Ctx *c, const AnalyzeCall &call, int h, int w, int K, const GraphParams &gp, TreeJob &tj)
{
    const size_t cper = (size_t)tj.cv.vh * tj.cv.vw * 3, fper = (size_t)gp.fh * gp.fw;
    tj.sf = (double)w / (double)gp.fw;
    tj.rgb_out = call.rgb_out; tj.bars_out = call.bars_out; tj.cap_b = call.cap_b; tj.n_bars = call.n_bars;
    tj.seg_cap = (size_t)K * fper;
    tj.bg_all = (uint16_t *)ws_get(c, WS_TREE_BG, (size_t)call.n * h * w * sizeof(uint16_t));
    tj.dseg = (OverlaySeg *)ws_get(c, WS_TREE_SEG, tj.seg_cap * sizeof(OverlaySeg));
    tj.dmm = (float *)ws_get(c, WS_TREE_MM, (size_t)K * 4 * sizeof(float) + (size_t)(K + 1) * sizeof(int));
    tj.drgb = (uint8_t *)ws_get(c, WS_TREE_RGB, (size_t)K * cper);
    if (!tj.bg_all || !tj.dseg || !tj.dmm || !tj.drgb) return TMAT_E_HIP;
    tj.doff = (int *)(tj.dmm + 4 * (size_t)K);
    if (tj.barcode_png) {       // rectangle tables (<= cap_b bars per image) and the K barcode canvases of a pass
        tj.drect = (BarRect *)ws_get(c, WS_GRID_BAR_RECT, (size_t)K * (size_t)call.cap_b * sizeof(BarRect) + (size_t)(K + 1) * sizeof(int) + 16);
        tj.dbar = (uint8_t *)ws_get(c, WS_GRID_BAR_RGB, (size_t)K * tj.S * tj.S * 3);
        if (!tj.drect || !tj.dbar) return TMAT_E_HIP;
        tj.drect_off = (int *)(tj.drect + (size_t)K * (size_t)call.cap_b);       // BarRect is five words: word-aligned
    }
    tj.png_mode = c->png_mode;
    if (tj.tree_png || tj.barcode_png) {        // encoder scratch (png.h:png_encode_launch) for the larger of the two shapes
        size_t filt = 0, slots = 0, files = 0, meta_words = 0, kp_max = 0;
        for (const PngShape *pg : {tj.tree_png ? &tj.pg_tree : nullptr, tj.barcode_png ? &tj.pg_bar : nullptr}) {
            if (!pg) continue;
            const size_t kp = (size_t)png_chunk(*pg, K);
            filt = std::max(filt, kp * pg->raw); slots = std::max(slots, kp * pg->ns * PNG_SLOT);
            files = std::max(files, kp * png_fcap(*pg)); meta_words = std::max(meta_words, kp * pg->ns * 4); kp_max = std::max(kp_max, kp);
        }
        tj.png_filt = (uint8_t *)ws_get(c, WS_GRID_PNG_FILT, filt); tj.png_slots = (uint8_t *)ws_get(c, WS_GRID_PNG_SLOTS, slots);
        tj.png_files = (uint8_t *)ws_get(c, WS_GRID_PNG_FILES, files);
        tj.png_meta = (uint32_t *)ws_get(c, WS_GRID_PNG_META, (meta_words + kp_max) * sizeof(uint32_t));     // the file sizes ride behind the stripe records
        if (!tj.png_filt || !tj.png_slots || !tj.png_files || !tj.png_meta) return TMAT_E_HIP;
        tj.png_dsz = tj.png_meta + meta_words;
    }
    return TMAT_OK;
}

// the well masks go up once per call, into a workspace of the handle; one seg buffer serves every pass (the tails share a stream)
static int well_setup(Ctx *c, const AnalyzeCall &call, int h, int w, int K, const uint8_t *&well_all, uint8_t *&seg)
{
    uint8_t *wd = (uint8_t *)ws_get(c, WS_WELL_MASK, (size_t)call.n * h * w);
    seg = (uint8_t *)ws_get(c, WS_WELL_SEG, (size_t)K * h * w);
    if (!wd || !seg) return TMAT_E_HIP;
    if (!hip_ok(hipMemcpy(wd, call.well, (size_t)call.n * h * w, hipMemcpyHostToDevice), "H2D(well masks)")) return TMAT_E_HIP;
    well_all = wd;
    return TMAT_OK;
}

// scratch of the stage pictures: tool workspaces as well, sized before any pass is in flight
static int stage_setup(Ctx *c, const AnalyzeCall &call, int h, int w, int K, StageJob &sj)
{
    sj.orig_all = (uint8_t *)ws_get(c, WS_STAGE_ORIG, (size_t)call.n * h * w);
    sj.pics = (uint8_t *)ws_get(c, WS_STAGE_PIC, 3 * (size_t)K * h * w);
    sj.mm = ws_get(c, WS_STAGE_MM, vis_scratch_bytes(K));
    if (!sj.orig_all || !sj.pics || !sj.mm) return TMAT_E_HIP;
    sj.out = call.stage_out; sj.K = K;
    return TMAT_OK;
}

// a checked call with its images on the device: geometry, buffers, the three set-up steps, the pass loop
static int analyze_dev(Ctx *c, const AnalyzeCall &call)
{
    const int n = call.n, H = call.H, W = call.W;
    tmat_row *rows = call.rows;
    // compute_branches.py:309-312 hands target_shape = round(shape * ds_ratio) = (round(H r), round(W r)) to cv2.resize as
    // dsize, which cv2 reads as (width, height): the resized image has round(W r) rows and round(H r) columns.  Square
    // images are unaffected; for the others the network sees the reference's (anisotropically scaled) image and the
    // later resize to (fh, fw) restores the aspect ratio, exactly as in the reference.
    const int h = round_half_even((double)W * call.ds_ratio), w = round_half_even((double)H * call.ds_ratio);
    if (h < 1 || w < 1) { set_error("analyze: target shape is empty"); return TMAT_E_ARG; }
    GraphParams gp = call.gp;
    gp.fh = round_half_even((double)H * ((double)call.ds_width / (double)W));
    gp.fw = round_half_even((double)W * ((double)call.ds_width / (double)W));
    const float one_pair[2] = {gp.t1, gp.t2};
    const GridJob gj{call.grid ? call.grid->n_thresh : 1, call.grid ? call.grid->thresh : one_pair, n};
    TreeJob tj{};
    StageJob sj{};
    TreeJob *tree = call.tree ? &tj : nullptr;
    StageJob *stage = call.stage_out ? &sj : nullptr;
    int rc = tree ? tree_shapes(call, h, w, tj) : TMAT_OK;
    if (rc) return rc;
    TileGeom g = make_geom(h, w, c->patch);
    roi_attach(c, g);       // region form of the up path: g carries the class-major patch order for enqueue_pre / enqueue_back
    const int K = std::min(n, std::max(1, c->max_patches / g.tiles_per_img));      // one image per pass when it needs > max_patches
    rc = ensure_patch_io(c, K * g.tiles_per_img);
    if (!rc) rc = ensure_pass_buffers(c, K, H, W, h, w, gp.fh, gp.fw);
    if (!rc) rc = ensure_ma_table(c);
    if (rc) return rc;
    for (size_t r = 0; r < (size_t)gj.T * n; r++) { rows[r].index = call.first_index + (int64_t)(r % (size_t)n); rows[r].count = 0; rows[r].total_px = 0; rows[r].avg_px = 0; }
    const uint8_t *well_all = nullptr, *pruning = call.pruning;
    uint8_t *seg = nullptr;
    if (tree) rc = tree_setup(c, call, h, w, K, gp, tj);
    if (!rc && call.well) rc = well_setup(c, call, h, w, K, well_all, seg);
    if (!rc && stage) rc = stage_setup(c, call, h, w, K, sj);
    if (rc) return rc;
    auto bg_at = [&](int p) { return tree ? tj.bg_all + (size_t)p * K * h * w : nullptr; };
    auto orig_at = [&](int p) { return stage ? sj.orig_all + (size_t)p * K * h * w : nullptr; };
    auto well_at = [&](int p) { return well_all ? well_all + (size_t)p * K * h * w : nullptr; };
    auto prune_at = [&](int p) { return pruning ? pruning + (size_t)p * K * gp.fh * gp.fw : nullptr; };
    const int P = (n + K - 1) / K;
    PassJob jobs[2];
    auto cnt = [&](int p) { return std::min(K, n - p * K); };
    auto img_at = [&](int p) { return call.imgs + (size_t)p * K * H * W; };
    // the caller may have queued work that produces the images on the main stream (tmat_zproj_dev, tmat_dev_upload)
    if (!use_one_stream() && !hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return TMAT_E_HIP;
    // second input buffer for the front end that runs ahead on the second stream (enqueue_pre)
    if (c->pre_side && tail_on_side_stream() && g.tiles_per_img <= c->max_patches && !c->patch_in2 &&
        !set_ptr(c->patch_in2, c->ws.dev((size_t)c->patch * c->patch * (c->patch_cap + c->const_cap) * sizeof(float), "hipMalloc(patch_in2)"))) return TMAT_E_HIP;
    if (pre_on_side_stream(c, g)) {         // what the caller queued on the main stream (the images) comes first on the second one too
        TMAT_HIP(hipEventRecord(c->ev_pre[0], c->stream));
        TMAT_HIP(hipStreamWaitEvent(c->stream2, c->ev_pre[0], 0));
    }
    // (order of the calls = order on the second stream: the front end of pass p + 2 in front of the tail of pass p + 1, which only
    // starts when that pass's up path has ended)
    c->down_pending[0] = c->down_pending[1] = false;
    rc = enqueue_pre(c, img_at(0), cnt(0), 0, g, bg_at(0), well_at(0), orig_at(0));
    if (!rc) rc = enqueue_down(c, cnt(0), 0, g);
    if (!rc && P > 1) rc = enqueue_pre(c, img_at(1), cnt(1), 1, g, bg_at(1), well_at(1), orig_at(1));
    if (!rc) rc = enqueue_back(c, cnt(0), 0, g, well_at(0), seg);
    if (!rc && P > 1) rc = enqueue_down(c, cnt(1), 1, g);
    for (int p = 0; p < P && !rc; p++) {
        const int slot = p & 1;
        const double tw0 = now_s();
        if (!hip_ok(hipEventSynchronize(c->pass.done[slot]), "hipEventSynchronize")) { rc = TMAT_E_HIP; break; }
        const double tw1 = now_s();
        if (p >= 1) { jobs[slot ^ 1].join(); if (jobs[slot ^ 1].rc) rc = jobs[slot ^ 1].rc; }
        if (trace_on())
            fprintf(stderr, "[tmat] pass %d/%d (%d images): waited %.1f ms for the GPU, %.1f ms for host jobs of the previous pass\n",
                    p + 1, P, cnt(p), (tw1 - tw0) * 1e3, (now_s() - tw1) * 1e3);
        if (p + 2 < P && !rc) rc = enqueue_pre(c, img_at(p + 2), cnt(p + 2), slot, g, bg_at(p + 2), well_at(p + 2), orig_at(p + 2));
        if (p + 1 < P && !rc) rc = enqueue_back(c, cnt(p + 1), slot ^ 1, g, well_at(p + 1), seg);
        if (p + 2 < P && !rc) rc = enqueue_down(c, cnt(p + 2), slot, g);
        for (int i = 0; i < cnt(p) && !rc; i++)
            if (!c->pass.conv_host[slot][i]) { set_error("analyze: Zhang thinning did not converge within its launch budget"); rc = TMAT_E_HIP; }
        if (!rc) jobs[slot].th = std::thread(run_pass_host, c, slot, cnt(p), gp, gj, rows, &jobs[slot], tree, p * K, prune_at(p), stage);
    }
    for (auto &j : jobs) { j.join(); if (j.rc && !rc) rc = j.rc; }
    hipStreamSynchronize(c->stream2);
    hipStreamSynchronize(c->stream);
    return rc;
}

// medial_axis on the device for k masks that are in HBM with their EDT: foreground counts -> host permutations -> keys,
// sort, ordered thinning (thin_kernels.hip).  Synchronises the stream once (the counts come back to the host).
// stages (test-only, tmat_debug_medial_stages; null for every other caller): host arrays, each of which may be null, that receive
// copies of what thin_dev left in its workspace.
struct ThinStages { uint64_t *keys; uint8_t *dep; int32_t *launches; };
static int medial_thin_stages_dev(Ctx *c, const uint8_t *mask_dev, const double *dist_dev, int k, int hh, int ww, uint8_t *skel_dev, hipStream_t s,
                                  const ThinStages *stages)
{
    int rc = ensure_ma_table(c);
    if (rc) return rc;
    const size_t per = (size_t)hh * ww;
    DevScope mem(c->ws_pool, s);
    int *nfg_host = mem.host<int>(k);
    int *nfg = mem.alloc<int>(k);
    // the permutations and the workspace come from the handle's pool: the next call of the same geometry gets the same blocks back, with
    // whatever this one left in them (tmat_debug_poison fills the pool) -- thin_dev's memset of its per-tile flags is what the
    // repeat-after-poison test holds
    uint32_t *tie = mem.pooled<uint32_t>(k * per);
    void *ws = mem.pooled_bytes(thin_workspace_bytes(k, hh, ww));
    if (!mem.ok || thin_count_dev(mask_dev, k, hh, ww, nfg, s)) return TMAT_E_HIP;
    mem.d2h(nfg_host, nfg, k * sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    std::vector<std::vector<uint32_t>> perms(k);
    parallel_images(k, [&](int i) { legacy_permutation(0, (size_t)nfg_host[i], perms[i]); });
    for (int i = 0; i < k; i++) {
        const size_t bytes = perms[i].size() * sizeof(uint32_t);
        if (bytes) mem.h2d(tie + i * per, mem.keep(std::move(perms[i])), bytes);
    }
    if (!mem.ok) return TMAT_E_HIP;
    int launches = 0;
    if (const int trc = thin_dev(mask_dev, dist_dev, tie, nfg, k, hh, ww, ws, c->ma_table, skel_dev, s, &launches)) {
        // -3: the launch budget is used up and pixels are still undone; -2: a HIP call failed
        set_error("medial axis: device thinning failed (" + std::to_string(trc) + " after " + std::to_string(launches) + " launches)");
        return TMAT_E_HIP;
    }
    if (stages) {
        const ThinLayout lay = thin_layout(ws, k, hh, ww);
        mem.d2h(stages->keys, lay.keys, k * per * sizeof(uint64_t));
        mem.d2h(stages->dep, lay.dep, k * per);
        if (stages->launches) *stages->launches = launches;
    }
    return mem.finish();
}

int medial_thin_batch_dev(Ctx *c, const uint8_t *mask_dev, const double *dist_dev, int k, int hh, int ww, uint8_t *skel_dev, hipStream_t s)
{
    return medial_thin_stages_dev(c, mask_dev, dist_dev, k, hh, ww, skel_dev, s, nullptr);
}

// tmat_dmt_graph / tmat_dmt_graph_batch with a handle: key build + sort + the two persistence sweeps of all n fields on the handle's
// device (one launch each), `collect` per field on host threads.  Outputs of field i start at verts + 2 i cap_v / edges + 2 i cap_e.
int dmt_graph_device_batch(void *handle, const float *imgs, int n, int R, int C, float delta1, float delta2, int32_t *verts, int cap_v,
                           int32_t *edges, int cap_e, int *n_verts, int *n_edges)
{
    Ctx *c = (Ctx *)handle;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t nE = dmt_edge_count(R, C), npx = (size_t)R * C;
    DevScope mem(c->ws_pool, c->stream);
    int32_t *ids_host = mem.host<int32_t>(n * nE);
    int *m_host = mem.host<int>(n);
    uint8_t *kind_host = nullptr;
    float *pers_host = nullptr;
    float *df = mem.alloc_from(imgs, n * npx);
    void *ws = mem.alloc_bytes(dmt_workspace_bytes(n, R, C));
    int32_t *ids = mem.alloc<int32_t>(n * nE);
    int *m = mem.alloc<int>(n);
    if (!mem.ok) return TMAT_E_HIP;
    if (dmt_sorted_edges_dev(df, n, R, C, ws, ids, m, c->stream)) { set_error("tmat_dmt_graph: device front end failed"); return TMAT_E_HIP; }
    // the two persistence sweeps on the device too (dmt_sweep_kernels.hip; TMAT_DMT_SWEEP_DEVICE=0: on the host); `collect` stays on the host
    if (c->dmt_sweep_device) {
        void *sws = mem.alloc_bytes(dmt_sweep_workspace_bytes(n, R, C));
        uint8_t *dkind = mem.alloc<uint8_t>(n * nE);
        float *dpers = mem.alloc<float>(n * nE);
        if (!mem.ok) return TMAT_E_HIP;
        if (dmt_sweeps_dev(df, ids, m, n, R, C, sws, dkind, dpers, c->stream)) { set_error("tmat_dmt_graph: device sweeps failed"); return TMAT_E_HIP; }
        mem.d2h(kind_host = mem.host<uint8_t>(n * nE), dkind, n * nE);
        mem.d2h(pers_host = mem.host<float>(n * nE), dpers, n * nE * sizeof(float));
    }
    mem.d2h(ids_host, ids, n * nE * sizeof(int32_t));
    mem.d2h(m_host, m, n * sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    std::vector<int> rcs(n, TMAT_OK);
    parallel_images(n, [&](int i) {
        rcs[i] = dmt_graph_host_sorted(imgs + i * npx, R, C, delta1, delta2, ids_host + i * nE, m_host[i], verts + (size_t)i * 2 * cap_v, cap_v,
                                       edges + (size_t)i * 2 * cap_e, cap_e, n_verts + i, n_edges + i, kind_host ? kind_host + i * nE : nullptr,
                                       pers_host ? pers_host + i * nE : nullptr);
    });
    for (int i = 0; i < n; i++) if (rcs[i]) return rcs[i];
    return TMAT_OK;
}

int dmt_graph_device_front(void *handle, const float *img, int R, int C, float delta1, float delta2, int32_t *verts, int cap_v,
                           int32_t *edges, int cap_e, int *n_verts, int *n_edges)
{
    return dmt_graph_device_batch(handle, img, 1, R, C, delta1, delta2, verts, cap_v, edges, cap_e, n_verts, n_edges);
}

}  // namespace tmat

using namespace tmat;

// The chunked entry points (tmat_segment_batch, tmat_preprocess_batch): the network's input shape (h, w) -- see analyze_dev --, K
// images per pass and the pass buffers; `name` heads the error text
static int chunked_setup(Ctx *c, const char *name, int n, int H, int W, double ds_ratio, int &h, int &w, int &K)
{
    h = round_half_even((double)W * ds_ratio); w = round_half_even((double)H * ds_ratio);
    if (h < 1 || w < 1) { set_error(std::string(name) + ": target shape is empty"); return TMAT_E_ARG; }
    const TileGeom g = make_geom(h, w, c->patch);
    K = std::min(n, std::max(1, c->max_patches / g.tiles_per_img));
    return ensure_pass_buffers(c, K, H, W, h, w, std::max(1, c->pass.fh), std::max(1, c->pass.fw));
}
// ... and their loop: the images go up K at a time through one staging buffer; pass(mem, dimg, i0, k) works on a chunk and ends with
// mem.finish()
template <class F>
static int chunked_upload(Ctx *c, const uint16_t *imgs, int n, int K, size_t per, F pass)
{
    DevScope mem(c->ws_pool, c->stream);
    uint16_t *dimg = mem.alloc<uint16_t>(K * per);
    int rc = mem.ok ? TMAT_OK : TMAT_E_HIP;
    for (int i0 = 0; i0 < n && !rc; i0 += K) {
        const int k = std::min(K, n - i0);
        rc = mem.h2d(dimg, imgs + i0 * per, k * per * sizeof(uint16_t)) ? pass(mem, dimg, i0, k) : TMAT_E_HIP;
    }
    return rc;
}

extern "C" {

int tmat_segment_batch(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, double ds_ratio, double *pred)
{
    Ctx *c = (Ctx *)hd;
    if (c && !has_model(c)) { set_error("tmat_segment_batch: this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (!c || !imgs || !pred || n < 0 || H < 1 || W < 1) { set_error("tmat_segment_batch: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    int h, w, K;
    int rc = chunked_setup(c, "tmat_segment_batch", n, H, W, ds_ratio, h, w, K);
    if (rc) return rc;
    return chunked_upload(c, imgs, n, K, (size_t)H * W, [&](DevScope &mem, const uint16_t *dimg, int i0, int k) {
        int rc = enqueue_segment(c, dimg, k, 0);
        if (!rc) rc = mem.finish();
        if (!rc) std::memcpy(pred + (size_t)i0 * h * w, c->pass.pred_host[0], (size_t)k * h * w * sizeof(double));
        return rc;
    });
}

int tmat_preprocess_batch(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, double ds_ratio, float *x)
{
    Ctx *c = (Ctx *)hd;
    if (c && !has_model(c)) { set_error("tmat_preprocess_batch: this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (!c || !imgs || !x || n < 0 || H < 1 || W < 1) { set_error("tmat_preprocess_batch: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    int h, w, K;
    int rc = chunked_setup(c, "tmat_preprocess_batch", n, H, W, ds_ratio, h, w, K);
    if (rc) return rc;
    PassBuf &b = c->pass;
    return chunked_upload(c, imgs, n, K, (size_t)H * W, [&](DevScope &mem, const uint16_t *dimg, int i0, int k) {
        launch_lanczos(dimg, k, b.H, b.W, b.h, b.w, b.xi, b.xc, b.yi, b.yc, b.tmp, b.small, c->input_sat, c->stream);
        launch_rescale01(b.small, k, (size_t)b.h * b.w, b.mn, b.mx, b.x, c->stream);
        mem.d2h(x + (size_t)i0 * h * w, b.x, (size_t)k * h * w * sizeof(float));
        return mem.finish();
    });
}

int tmat_filter_edt_batch(tmat_handle hd, const double *pred, int n, int hh, int ww, uint8_t *filtered, double *dist)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !pred || !filtered || !dist || n < 0 || hh < 1 || ww < 1) { set_error("tmat_filter_edt_batch: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)n * hh * ww;
    DevScope mem(c->ws_pool, c->stream);
    int *conv = mem.host<int>(n);
    double *dp = mem.alloc_from(pred, npx), *dd = mem.alloc<double>(npx);
    uint8_t *df = mem.alloc<uint8_t>(npx);
    void *ws = mem.alloc_bytes(morph_workspace_bytes(n, hh, ww));
    if (!mem.ok || filter_edt_dev(dp, n, hh, ww, 1, ws, df, dd, c->stream)) return TMAT_E_HIP;
    mem.d2h(filtered, df, npx);
    mem.d2h(dist, dd, npx * 8);
    mem.d2h(conv, morph_done_flags(ws, n, hh, ww), n * sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    for (int i = 0; i < n; i++) if (!conv[i]) { set_error("tmat_filter_edt_batch: thinning did not converge"); return TMAT_E_HIP; }
    return TMAT_OK;
}

int tmat_filter_mask_batch(tmat_handle hd, const uint8_t *mask, int n, int hh, int ww, int use_median, int remove_isolated, uint8_t *filtered)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !mask || !filtered || n < 0 || hh < 1 || ww < 1) { set_error("tmat_filter_mask_batch: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)n * hh * ww;
    DevScope mem(c->ws_pool, c->stream);
    int *conv = mem.host<int>(n);
    uint8_t *dm = mem.alloc_from(mask, npx), *df = mem.alloc<uint8_t>(npx);
    void *ws = mem.alloc_bytes(morph_workspace_bytes(n, hh, ww));
    if (!mem.ok || filter_mask_dev(nullptr, dm, n, hh, ww, use_median != 0, remove_isolated != 0, ws, df, nullptr, c->stream)) return TMAT_E_HIP;
    mem.d2h(filtered, df, npx);
    mem.d2h(conv, morph_done_flags(ws, n, hh, ww), n * sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    for (int i = 0; i < n; i++) if (!conv[i]) { set_error("tmat_filter_mask_batch: thinning did not converge"); return TMAT_E_HIP; }
    return TMAT_OK;
}

// Test-only (tests/test_gpu_morph_stages.py): tmat_filter_mask_batch's call of filter_mask_dev, plus copies of what its workspace holds
int tmat_debug_filter_stages(tmat_handle hd, const uint8_t *mask, int n, int hh, int ww, int use_median, int remove_isolated, uint8_t *median,
                             int32_t *labels, int32_t *stats, uint8_t *skeleton, uint8_t *filtered, int32_t *thin_launches)
{
    Ctx *c = (Ctx *)hd;
    const bool any_out = median || labels || stats || skeleton || filtered || thin_launches;
    if (!c || !mask || !any_out || n < 0 || hh < 1 || ww < 1) { set_error("tmat_debug_filter_stages: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t per = (size_t)hh * ww, npx = (size_t)n * per;
    DevScope mem(c->ws_pool, c->stream);
    int *conv = mem.host<int>(n);
    uint8_t *dm = mem.alloc_from(mask, npx), *df = mem.alloc<uint8_t>(npx);
    void *ws = mem.alloc_bytes(morph_workspace_bytes(n, hh, ww));
    if (!mem.ok || filter_mask_dev(nullptr, dm, n, hh, ww, use_median != 0, remove_isolated != 0, ws, df, nullptr, c->stream)) return TMAT_E_HIP;
    const MorphLayout lay = morph_layout(ws, n, hh, ww);
    int *chg = mem.host<int>((size_t)lay.launches * n);
    mem.d2h(median, lay.med, npx);
    mem.d2h(labels, lay.ML, npx * sizeof(int));
    for (int i = 0; i < n && stats; i++) {           // area, n1, n2, n3 are consecutive (n, H, W) planes -> (n, 4, H, W)
        const int *planes[4] = {lay.area, lay.n1, lay.n2, lay.n3};
        for (int j = 0; j < 4; j++) mem.d2h(stats + ((size_t)i * 4 + j) * per, planes[j] + (size_t)i * per, per * sizeof(int));
    }
    mem.d2h(skeleton, lay.skA, npx);
    mem.d2h(filtered, df, npx);
    mem.d2h(chg, lay.changed, (size_t)lay.launches * n * sizeof(int));
    mem.d2h(conv, lay.done, n * sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    for (int i = 0; i < n && thin_launches; i++) {
        thin_launches[i] = 0;
        for (int it = 0; it < lay.launches; it++) thin_launches[i] += chg[(size_t)it * n + i] != 0;
    }
    for (int i = 0; i < n; i++) if (!conv[i]) { set_error("tmat_debug_filter_stages: thinning did not converge"); return TMAT_E_HIP; }
    return TMAT_OK;
}

int tmat_finish_batch(tmat_handle hd, const double *pred, const double *dist, const uint8_t *skel, int n, int hh, int ww, int out_h,
                      int out_w, float *field, float *field255)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !pred || !dist || !skel || !field || !field255 || n < 0 || hh < 1 || ww < 1 || out_h < 1 || out_w < 1) {
        set_error("tmat_finish_batch: bad argument");
        return TMAT_E_ARG;
    }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)n * hh * ww, onpx = (size_t)n * out_h * out_w;
    DevScope mem(c->ws_pool, c->stream);
    double *dp = mem.alloc_from(pred, npx), *dd = mem.alloc_from(dist, npx);
    uint8_t *ds = mem.alloc_from(skel, npx);
    void *ws = mem.alloc_bytes(finish_workspace_bytes(n, hh, ww, out_h, out_w));
    float *df = mem.alloc<float>(onpx), *d255 = mem.alloc<float>(onpx);
    if (!mem.ok || finish_dev(dp, dd, ds, n, hh, ww, out_h, out_w, ws, df, d255, c->stream)) return TMAT_E_HIP;
    mem.d2h(field, df, onpx * 4);
    mem.d2h(field255, d255, onpx * 4);
    return mem.finish();
}

int tmat_zproj_dev(tmat_handle hd, const uint16_t *stacks_dev, int n, int Z, int H, int W, int method, void *out_dev)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !stacks_dev || !out_dev || n < 0 || Z < 1 || H < 1 || W < 1 || method < TMAT_ZPROJ_FS || method > TMAT_ZPROJ_MED) {
        set_error("tmat_zproj_dev: bad argument");
        return TMAT_E_ARG;
    }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const int rc = zproj_dev(stacks_dev, n, Z, H, W, method, out_dev, c->stream);
    return rc == 0 ? TMAT_OK : rc == -1 ? TMAT_E_ARG : TMAT_E_HIP;
}

int tmat_zproj_batch(tmat_handle hd, const uint16_t *stacks, int n, int Z, int H, int W, int method, void *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !stacks || !out || n < 0 || Z < 1 || H < 1 || W < 1 || method < TMAT_ZPROJ_FS || method > TMAT_ZPROJ_MED) {
        set_error("tmat_zproj_batch: bad argument");
        return TMAT_E_ARG;
    }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)H * W, per_in = (size_t)Z * npx * sizeof(uint16_t);
    const size_t osz = (method == TMAT_ZPROJ_AVG || method == TMAT_ZPROJ_MED) ? sizeof(double) : sizeof(uint16_t);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)1 << 30) / per_in));   // <= 1 GiB of stacks at a time
    // the staging buffers stay on the handle between calls (tmat_ctx.h:ws_get); the scope only carries the copies
    uint16_t *din = (uint16_t *)ws_get(c, WS_ZPROJ_IN, (size_t)chunk * per_in);
    void *dout = ws_get(c, WS_ZPROJ_OUT, (size_t)chunk * npx * osz);
    if (!din || !dout) return TMAT_E_HIP;
    DevScope mem(c->ws_pool, c->stream);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int k = std::min(chunk, n - i0);
        if (!mem.h2d(din, stacks + (size_t)i0 * Z * npx, (size_t)k * per_in)) return TMAT_E_HIP;
        const int r = zproj_dev(din, k, Z, H, W, method, dout, c->stream);
        if (r) return r == -1 ? TMAT_E_ARG : TMAT_E_HIP;
        mem.d2h((char *)out + (size_t)i0 * npx * osz, dout, (size_t)k * npx * osz);
        if (mem.finish()) return TMAT_E_HIP;
    }
    return TMAT_OK;
}

// The post-processing of compute_branches.py:334-357 for a batch of probability maps, with the same split as the batch
// pipeline: GPU (threshold, filter_branch_seg_mask, EDT) -> host (ordered medial-axis thinning, sequential by
// construction) -> GPU (EDT of the skeleton, weighting, anti-aliased resize).  Chunked to bound device memory.
int tmat_postprocess_batch(tmat_handle hd, const double *pred, int n, int hh, int ww, int out_h, int out_w, float *field)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !pred || !field || n < 0 || hh < 1 || ww < 1 || out_h < 1 || out_w < 1) { set_error("tmat_postprocess_batch: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t per = (size_t)hh * ww, oper = (size_t)out_h * out_w;
    const int K = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / (per * 8)));      // <= 256 MiB of f64 maps per chunk
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    uint8_t *filt = mem.host<uint8_t>(K * per), *skel = mem.host<uint8_t>(K * per);
    double *dist = mem.host<double>(K * per);
    int *conv = mem.host<int>(K);
    double *dp = mem.alloc<double>(K * per), *dd = mem.alloc<double>(K * per);
    uint8_t *df = mem.alloc<uint8_t>(K * per), *dsk = mem.alloc<uint8_t>(K * per);
    void *ws = mem.alloc_bytes(morph_workspace_bytes(K, hh, ww)), *fws = mem.alloc_bytes(finish_workspace_bytes(K, hh, ww, out_h, out_w));
    float *dfield = mem.alloc<float>(K * oper), *d255 = mem.alloc<float>(K * oper);
    if (!mem.ok) return TMAT_E_HIP;
    for (int i0 = 0; i0 < n; i0 += K) {
        const int k = std::min(K, n - i0);
        if (!mem.h2d(dp, pred + (size_t)i0 * per, k * per * 8) || filter_edt_dev(dp, k, hh, ww, 1, ws, df, dd, s)) return TMAT_E_HIP;
        mem.d2h(filt, df, k * per);
        mem.d2h(dist, dd, k * per * 8);
        mem.d2h(conv, morph_done_flags(ws, k, hh, ww), k * sizeof(int));
        if (mem.finish()) return TMAT_E_HIP;
        for (int i = 0; i < k; i++) if (!conv[i]) { set_error("tmat_postprocess_batch: thinning did not converge"); return TMAT_E_HIP; }
        if (c->thin_device && thin_dev_supported(hh, ww)) {
            int rc = medial_thin_batch_dev(c, df, dd, k, hh, ww, dsk, s);
            if (rc) return rc;
        } else {        // images too large for the LDS-resident thinning kernel: host threads
            parallel_images(k, [&](int i) { medial_axis_thin(filt + i * per, dist + i * per, hh, ww, skel + i * per); });
            if (!mem.h2d(dsk, skel, k * per)) return TMAT_E_HIP;
        }
        if (finish_dev(dp, dd, dsk, k, hh, ww, out_h, out_w, fws, dfield, d255, s)) return TMAT_E_HIP;
        mem.d2h(field + (size_t)i0 * oper, dfield, k * oper * 4);
        if (mem.finish()) return TMAT_E_HIP;
    }
    return TMAT_OK;
}

// tmat_medial_axis_batch and, with `stages`, tmat_debug_medial_stages: one body, so that the test-only entry point cannot drift
// from the one it looks into.  The caller has checked its arguments; skel and dist may be null with stages.
static int medial_axis_entry(Ctx *c, const char *name, const uint8_t *mask, int n, int hh, int ww, uint8_t *skel, double *dist, const ThinStages *stages)
{
    if (n == 0) return TMAT_OK;
    if (!thin_dev_supported(hh, ww)) { set_error(std::string(name) + ": image too large for the device thinning kernel (use tmat_host_medial_axis)"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)n * hh * ww;
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    uint8_t *dm = mem.alloc_from(mask, npx), *dsk = mem.alloc<uint8_t>(npx);
    double *dd = mem.alloc<double>(npx);
    int *g = mem.alloc<int>(npx), *anyz = mem.alloc<int>(n);
    if (!mem.ok) return TMAT_E_HIP;
    launch_edt(dm, n, hh, ww, g, nullptr, anyz, dd, s);
    int rc = medial_thin_stages_dev(c, dm, dd, n, hh, ww, dsk, s, stages);
    if (rc) return rc;
    mem.d2h(skel, dsk, npx);
    mem.d2h(dist, dd, npx * 8);
    return mem.finish();
}

int tmat_medial_axis_batch(tmat_handle hd, const uint8_t *mask, int n, int hh, int ww, uint8_t *skel, double *dist)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !mask || !skel || !dist || n < 0 || hh < 1 || ww < 1) { set_error("tmat_medial_axis_batch: bad argument"); return TMAT_E_ARG; }
    return medial_axis_entry(c, "tmat_medial_axis_batch", mask, n, hh, ww, skel, dist, nullptr);
}

// Test-only (tests/test_gpu_medial_stages.py): tmat_medial_axis_batch's calls, plus copies of what thin_dev's workspace holds
int tmat_debug_medial_stages(tmat_handle hd, const uint8_t *mask, int n, int hh, int ww, uint8_t *skel, double *dist, uint64_t *keys, uint8_t *dep,
                             int32_t *launches)
{
    Ctx *c = (Ctx *)hd;
    const bool any_out = skel || dist || keys || dep || launches;
    if (!c || !mask || !any_out || n < 0 || hh < 1 || ww < 1) { set_error("tmat_debug_medial_stages: bad argument"); return TMAT_E_ARG; }
    const ThinStages stages{keys, dep, launches};
    return medial_axis_entry(c, "tmat_debug_medial_stages", mask, n, hh, ww, skel, dist, &stages);
}

// The 2-D batch analysis family: nine entry points, one path.  Each fills an AnalyzeCall and hands it to analyze_entry.

// the one complete argument check, the same for host and device images
static bool analyze_args_ok(const Ctx *c, const AnalyzeCall &call)
{
    const tmat_grid_opts *g = call.grid;
    const bool png = g && (g->tree_png || g->barcode_png);
    return c && call.imgs && call.rows && call.n >= 0 && call.H >= 1 && call.W >= 1 && call.ds_width >= 1 &&
           (!call.tree || (call.vis_width >= 1 && call.bars_out && call.cap_b >= 0 && call.n_bars && (call.rgb_out || png))) &&
           (!g || ((!g->tree_png || g->tree_png_sizes) && (!g->barcode_png || g->barcode_png_sizes)));
}

// model, arguments, n == 0, device, upload of host images, analyze_dev -- in this order: a refused call has touched nothing
static int analyze_entry(tmat_handle hd, const AnalyzeCall &call)
{
    Ctx *c = (Ctx *)hd;
    const std::string name = call.name;
    if (c && !has_model(c)) { set_error(name + ": this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (call.grid && (call.grid->n_thresh < 1 || !call.grid->thresh)) { set_error(name + ": n_thresh < 1 or no thresholds"); return TMAT_E_ARG; }
    if (!analyze_args_ok(c, call)) { set_error(name + ": bad argument"); return TMAT_E_ARG; }
    if (call.n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    if (!call.host) return analyze_dev(c, call);
    DevScope mem(c->ws_pool, nullptr);       // blocking copy below: nothing to drain
    const size_t px = (size_t)call.n * call.H * call.W;
    uint16_t *dimg = mem.alloc<uint16_t>(px);
    if (!mem.ok) return TMAT_E_HIP;
    if (!hip_ok(hipMemcpy(dimg, call.imgs, px * 2, hipMemcpyHostToDevice), "H2D")) return TMAT_E_HIP;
    AnalyzeCall dev = call;
    dev.imgs = dimg;
    return analyze_dev(c, dev);
}

// the extensible forms: the structs' sizes are checked here, where they are first read and before any field is touched
static int analyze_entry_opts(const char *name, tmat_handle hd, const uint16_t *imgs, bool host, int n, int H, int W, const tmat_analyze_opts *o,
                              const tmat_grid_opts *g, bool grid_form, tmat_row *rows)
{
    if (!o || o->size != (uint32_t)sizeof(tmat_analyze_opts)) { set_error(std::string(name) + ": unknown tmat_analyze_opts size"); return TMAT_E_ARG; }
    if (grid_form && (!g || g->size != (uint32_t)sizeof(tmat_grid_opts))) { set_error(std::string(name) + ": unknown tmat_grid_opts size"); return TMAT_E_ARG; }
    const bool tree = o->rgb_out || (g && (g->tree_png || g->barcode_png));
    return analyze_entry(hd, AnalyzeCall{name, imgs, host, n, H, W, o->ds_ratio, o->ds_width,
                                         {0, 0, o->graph_thresh_1, o->graph_thresh_2, o->smoothing_window_px, o->min_branch_length_px, o->max_branch_length_px, o->remove_isolated},
                                         o->first_index, rows, tree, o->vis_width, o->rgb_out, o->bars_out, o->cap_b, o->n_bars, o->well_masks, o->pruning_masks,
                                         o->stage_out, g});
}

int tmat_analyze_batch(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, double ds_ratio, int ds_width,
                       float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                       int max_branch_length_px, int remove_isolated, int64_t first_index, tmat_row *rows)
{
    AnalyzeCall call{"tmat_analyze_batch", imgs, true, n, H, W, ds_ratio, ds_width,
                  {0, 0, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated},
                  first_index, rows};
    return analyze_entry(hd, call);
}

int tmat_analyze_batch_dev(tmat_handle hd, const uint16_t *imgs_dev, int n, int H, int W, double ds_ratio, int ds_width,
                           float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                           int max_branch_length_px, int remove_isolated, int64_t first_index, tmat_row *rows)
{
    AnalyzeCall call{"tmat_analyze_batch_dev", imgs_dev, false, n, H, W, ds_ratio, ds_width,
                  {0, 0, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated},
                  first_index, rows};
    return analyze_entry(hd, call);
}

int tmat_analyze_batch_masked(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, double ds_ratio, int ds_width,
                              float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                              int max_branch_length_px, int remove_isolated, int64_t first_index, const uint8_t *well_masks,
                              const uint8_t *pruning_masks, tmat_row *rows)
{
    AnalyzeCall call{"tmat_analyze_batch_masked", imgs, true, n, H, W, ds_ratio, ds_width,
                  {0, 0, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated},
                  first_index, rows};
    call.well = well_masks; call.pruning = pruning_masks;
    return analyze_entry(hd, call);
}

int tmat_analyze_batch_tree(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, double ds_ratio, int ds_width,
                            float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                            int max_branch_length_px, int remove_isolated, int64_t first_index, tmat_row *rows, int vis_width,
                            uint8_t *rgb_out, double *bars_out, int cap_b, int *n_bars)
{
    AnalyzeCall call{"tmat_analyze_batch_tree", imgs, true, n, H, W, ds_ratio, ds_width,
                  {0, 0, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated},
                  first_index, rows};
    call.tree = true; call.vis_width = vis_width; call.rgb_out = rgb_out; call.bars_out = bars_out; call.cap_b = cap_b; call.n_bars = n_bars;
    return analyze_entry(hd, call);
}

int tmat_analyze_batch_tree_dev(tmat_handle hd, const uint16_t *imgs_dev, int n, int H, int W, double ds_ratio, int ds_width,
                                float graph_thresh_1, float graph_thresh_2, int smoothing_window_px, int min_branch_length_px,
                                int max_branch_length_px, int remove_isolated, int64_t first_index, tmat_row *rows, int vis_width,
                                uint8_t *rgb_out, double *bars_out, int cap_b, int *n_bars)
{
    AnalyzeCall call{"tmat_analyze_batch_tree_dev", imgs_dev, false, n, H, W, ds_ratio, ds_width,
                  {0, 0, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated},
                  first_index, rows};
    call.tree = true; call.vis_width = vis_width; call.rgb_out = rgb_out; call.bars_out = bars_out; call.cap_b = cap_b; call.n_bars = n_bars;
    return analyze_entry(hd, call);
}

int tmat_analyze_batch_ex(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, const tmat_analyze_opts *o, tmat_row *rows)
{
    return analyze_entry_opts("tmat_analyze_batch_ex", hd, imgs, true, n, H, W, o, nullptr, false, rows);
}

int tmat_analyze_batch_ex_dev(tmat_handle hd, const uint16_t *imgs_dev, int n, int H, int W, const tmat_analyze_opts *o, tmat_row *rows)
{
    return analyze_entry_opts("tmat_analyze_batch_ex_dev", hd, imgs_dev, false, n, H, W, o, nullptr, false, rows);
}

int tmat_analyze_batch_grid(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, const tmat_analyze_opts *o, const tmat_grid_opts *g, tmat_row *rows)
{
    return analyze_entry_opts("tmat_analyze_batch_grid", hd, imgs, true, n, H, W, o, g, true, rows);
}

int tmat_analyze_batch_grid_dev(tmat_handle hd, const uint16_t *imgs_dev, int n, int H, int W, const tmat_analyze_opts *o, const tmat_grid_opts *g, tmat_row *rows)
{
    return analyze_entry_opts("tmat_analyze_batch_grid_dev", hd, imgs_dev, false, n, H, W, o, g, true, rows);
}

// a (n, per) of dtype TMAT_PIC_* -> out (n, per) u8: extrema and picture kernels of vis_kernels.hip, chunked to bound device memory
int tmat_stage_pictures(tmat_handle hd, const void *a, int dtype, int n, size_t per, uint8_t *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !a || !out || n < 0 || per < 1 || dtype < TMAT_PIC_U16 || dtype > TMAT_PIC_U8) { set_error("tmat_stage_pictures: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    static const size_t esz[4] = {2, 4, 8, 1};
    const size_t in_bytes = per * esz[dtype];
    const int K = (int)std::max<size_t>(1, std::min<size_t>(std::min(n, 65535), ((size_t)256 << 20) / in_bytes));     // <= 256 MiB of input per chunk
    DevScope mem(c->ws_pool, c->stream);
    void *da = mem.alloc_bytes((size_t)K * in_bytes);
    uint8_t *dout = mem.alloc<uint8_t>((size_t)K * per);
    void *mm = mem.alloc_bytes(vis_scratch_bytes(K));
    if (!mem.ok) return TMAT_E_HIP;
    for (int i0 = 0; i0 < n; i0 += K) {
        const int k = std::min(K, n - i0);
        if (!mem.h2d(da, (const char *)a + (size_t)i0 * in_bytes, (size_t)k * in_bytes)) return TMAT_E_HIP;
        double *lo = vis_scratch_lo(mm, k);
        if (vis_minmax_dev(da, dtype, k, per, mm, c->stream) || vis_picture_dev(da, dtype, k, per, lo, lo + k, dout, c->stream)) {
            set_error("tmat_stage_pictures: kernel launch failed");
            return TMAT_E_HIP;
        }
        mem.d2h(out + (size_t)i0 * per, dout, (size_t)k * per);
        if (mem.finish()) return TMAT_E_HIP;
    }
    return TMAT_OK;
}

}  // extern "C"
