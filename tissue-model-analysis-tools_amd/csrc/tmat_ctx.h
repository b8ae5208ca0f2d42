// Handle state of libtmat_hip.so.
#pragma once
#include "tmat_internal.h"
#include "dev_mem.h"
#include "gauss_tables.h"
#include "roi_plan.h"

#include <map>

namespace tmat {

struct DownBlock {
    int cin = 0, cout = 0;
    float *dw[2] = {nullptr, nullptr};      // [9][C]
    float *pw[2] = {nullptr, nullptr};      // [Cout][Cin] (k contiguous: conv_mfma_kernel and the fused separable kernel)
    float *scale[2] = {nullptr, nullptr}, *shift[2] = {nullptr, nullptr};
    float *res_w = nullptr, *res_b = nullptr;
};
struct UpBlock {
    int cin = 0, cout = 0;
    float *ct[2] = {nullptr, nullptr};      // conv-form taps [9][Cin][Cout]
    float *ct_sub = nullptr;                // first conv in sub-pixel form [4][4][Cin][Cout] (blocks after the first)
    float *scale[2] = {nullptr, nullptr}, *shift[2] = {nullptr, nullptr};
    float *res_w = nullptr, *res_b = nullptr;
};
struct ProfEv { hipEvent_t e0, e1; double flops; };
// tile table of a fused separable layer for passes of k images under a form (roi_plan.h:roi_sep_tile_table): dev (null: every patch whole,
// the launch stays full-frame) holds n ids; a constant like `order` -- uploaded once, outside the workspaces tmat_debug_poison fills
// form: ROI_DOWN_REGION, ROI_DOWN_CONST or ROI_DOWN_SHARE (the forms above it keep its tiles).  From ROI_DOWN_CONST upwards the table is
// followed by every tile of the pass's k all-constant patches, which sit behind its patches; n_rep of full_rep: the planner's own
// counts, without those (what tmat_debug_sep_tiles reports)
// quad: the quadrant table of a fused layer instead (roi_plan.h:roi_sep_quad_table for a plain layer, roi_sep_quad_pool_table for a pooled
// one): dev holds n packed tiles of four quadrant ids, the constant patches' included; n_rep the packed tiles of the pass's own patches,
// full and full_rep their full-frame tiles
struct RoiTileTab {
    int layer = 0, k = 0, n = 0; long long full = 0; int *dev = nullptr; RoiDownForm form = ROI_DOWN_REGION; long long n_rep = 0, full_rep = 0;
    bool quad = false;
};
// the neighbour copies of passes of k images under a form (ROI_DOWN_SHARE and above): the neighbour table in the pass's class-major
// order and, per stored tensor (layer), the items that form copies (roi_plan.h:roi_down_copy_items) -- host copies for the launcher's
// checks, device copies (uploaded once, like the tile tables) for the kernel
struct RoiShareTab {
    int k = 0;
    RoiDownForm form = ROI_DOWN_SHARE;
    std::vector<int> nbr;
    int *nbr_dev = nullptr;
    struct Layer { int layer = 0; std::vector<ShareItem> items; ShareItem *dev = nullptr; };
    std::vector<Layer> layers;
};
struct RoiEntry {
    RoiPlan plan;
    int4 *order = nullptr;                  // device, [tiles_per_img] (TileGeom::order)
    std::vector<RoiTileTab> tabs;           // made on first use; released when the handle moves to another geometry, and by tmat_destroy
    std::vector<RoiShareTab> shares;        // likewise
    void free_tabs()
    {
        for (RoiTileTab &t : tabs) if (t.dev) hipFree(t.dev);
        tabs.clear();
        for (RoiShareTab &t : shares) {
            if (t.nbr_dev) hipFree(t.nbr_dev);
            for (RoiShareTab::Layer &l : t.layers) if (l.dev) hipFree(l.dev);
        }
        shares.clear();
    }
};
struct ConvWHost { std::vector<float> w; int cin; };        // host copy of an MFMA convolution's weights ([rows][cin])

// per-geometry buffers of the batch pipeline (pipeline.cpp)
struct PassBuf {
    int K = 0, H = 0, W = 0, h = 0, w = 0;
    int *xi = nullptr, *yi = nullptr;
    float *xc = nullptr, *yc = nullptr;
    float *tmp = nullptr, *x = nullptr;
    uint16_t *small = nullptr;
    int *mn = nullptr, *mx = nullptr;
    double *pred[2] = {nullptr, nullptr};
    double *pred_host[2] = {nullptr, nullptr};
    // GPU morphology outputs (morph_kernels.hip): filtered mask, its EDT, per-image convergence flags
    void *morph_ws = nullptr;
    uint8_t *filt[2] = {nullptr, nullptr};
    double *dist[2] = {nullptr, nullptr};
    uint8_t *filt_host[2] = {nullptr, nullptr};
    double *dist_host[2] = {nullptr, nullptr};
    int *conv_host[2] = {nullptr, nullptr};
    // finish stage (finish_kernels.hip): skeleton from the host thinning, vesselness field back to the host
    int fh = 0, fw = 0;
    void *finish_ws = nullptr;
    uint8_t *skel[2] = {nullptr, nullptr};
    uint8_t *skel_host[2] = {nullptr, nullptr};
    float *field[2] = {nullptr, nullptr}, *f255[2] = {nullptr, nullptr};
    float *f255_host[2] = {nullptr, nullptr};
    // ordered thinning on the device (thin_kernels.hip): foreground counts, RandomState(0) permutations (host-made), scratch
    void *thin_ws = nullptr;
    int *nfg[2] = {nullptr, nullptr};
    int *nfg_host[2] = {nullptr, nullptr};
    uint32_t *tie = nullptr;
    uint32_t *tie_host[2] = {nullptr, nullptr};
    // DMT front end (dmt_kernels.hip): lower-star sorted edge ids of every image of the pass, counts of kept edges
    void *dmt_ws = nullptr;
    int32_t *dmt_ids[2] = {nullptr, nullptr};
    int32_t *dmt_ids_host[2] = {nullptr, nullptr};
    int *dmt_m[2] = {nullptr, nullptr};
    int *dmt_m_host[2] = {nullptr, nullptr};
    // the two persistence sweeps on the device (dmt_sweep_kernels.hip): pairing kind and persistence of every sorted edge
    void *dmt_sweep_ws = nullptr;
    uint8_t *dmt_kind[2] = {nullptr, nullptr};
    uint8_t *dmt_kind_host[2] = {nullptr, nullptr};
    float *dmt_pers[2] = {nullptr, nullptr};
    float *dmt_pers_host[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    WsList ws;                                              // owns every scratch allocation above (not the Lanczos tables: they are constants)
};

// weight container ("TMATW001", tmat_amd/synth.py:pack_weights): tensors by name, pointing into the caller's blob
struct Tensor { std::vector<int> shape; const float *data; size_t count; };
bool parse_blob(const void *blob, size_t nbytes, std::map<std::string, Tensor> &out, int &patch);
std::vector<float> k_contiguous(const float *w, int taps, int I, int O);        // [taps][I][O] -> [taps][O][I]

// ResNet50 classifier of the invasion-depth tool (resnet_kernels.hip)
struct ResConv {
    int cin = 0, cout = 0, ksize = 1, stride = 1;
    float *w = nullptr, *scale = nullptr, *shift = nullptr;
    void *w16 = nullptr;      // the same [tap][Cout][Cin] tensor as one IEEE f16 plane (TMAT_RESNET_PRECISION_F16; made when the mode is first on)
};
struct ResBlock { ResConv c1, c2, c3, sc; bool has_sc = false; };
struct ResNetModel {
    float *stem_w = nullptr, *stem_scale = nullptr, *stem_shift = nullptr;      // [147][64], folded BN
    void *stem_w16 = nullptr;                                                   // f16 plane of stem_w (see ResConv::w16)
    bool has_f16 = false;                                                       // every w16 / stem_w16 of the model is made (they are in `owned`)
    std::vector<ResBlock> blocks;
    float *fc_w = nullptr;
    float fc_b = 0.f;
    int feat = 0;                                                               // channels of the last block
    std::vector<void *> owned;
};

struct GaussKey {
    double sigma; int order, radius;
    bool operator<(const GaussKey &o) const { return sigma != o.sigma ? sigma < o.sigma : order != o.order ? order < o.order : radius < o.radius; }
};

// slots of ws_get: one per buffer of a side tool.  The overlay and tree slots are shared by tmat_render_tree (overlay.cpp) and the
// "with tree" form of tmat_analyze_batch_tree* (pipeline.cpp): both hold them for one call only, synchronise before they return, and
// a handle runs one entry point at a time, so the two are never live together.
enum ToolWs {
    WS_CELL_IN, WS_CELL_HIST, WS_CELL_KEPT, WS_CELL_PAR, WS_CELL_THR, WS_CELL_SMALL, WS_CELL_TAB, WS_CELL_MASK, WS_CELL_LOHI,       // cell area
    WS_ZPROJ_IN, WS_ZPROJ_OUT,                                                                                                      // Z projection
    WS_INV_IN, WS_INV_SMALL, WS_INV_TAB, WS_INV_MNMX, WS_INV_X, WS_INV_PROB, WS_INV_BUF0, WS_INV_BUF1, WS_INV_BUF2, WS_INV_BUF3,    // invasion depth
    WS_INV_COL,
    WS_TREE_BG, WS_TREE_SEG, WS_TREE_MM, WS_TREE_RGB,                                                                               // tree overlay
    WS_WELL_MASK, WS_WELL_SEG,                                                                                                      // masked batch pipeline
    WS_STAGE_ORIG, WS_STAGE_PIC, WS_STAGE_MM,                                                                                       // stage pictures of the batch pipeline
    WS_GRID_BAR_RECT, WS_GRID_BAR_RGB, WS_GRID_PNG_FILT, WS_GRID_PNG_SLOTS, WS_GRID_PNG_FILES, WS_GRID_PNG_META,                    // pictures of the grid form (tmat_analyze_batch_grid*)
    N_TOOL_WS
};

// An open smooth-tiling session (smooth_kernels.hip: tmat_smooth_begin ... tmat_smooth_end): the uploaded image, its minimum, the window
// and the predictions the caller has put so far.  It lives across calls and holds the caller's data, so it is no workspace:
// tmat_debug_poison leaves it alone; `mem` owns every block and tmat_smooth_end, the next begin and tmat_destroy release them.
struct SmoothSession {
    bool open = false;
    SmoothGeom g{};
    float *x = nullptr, *padval = nullptr;      // (hh, ww); [min, max]
    double *win = nullptr;                      // [ws]
    void *pred = nullptr;                       // (n_tiles, ws, ws), made by the first put
    bool pred_f64 = false;
    std::vector<uint8_t> have;                  // per tile: put
    WsList mem;
    hipEvent_t ev[2] = {nullptr, nullptr};      // around the last kernel launch
    double tiles_ms = 0, blend_ms = 0;          // device time of the gather launches / the blend of the last session (tmat_debug_smooth_times)
    void close()
    {
        mem.free_all();
        x = padval = nullptr; win = nullptr; pred = nullptr; pred_f64 = false; have.clear(); open = false;
    }
};

struct Ctx {
    int device = 0;
    SmoothSession smooth;
    std::vector<ResNetModel> resnets;                        // invasion-depth classifiers loaded on this handle (tmat_resnet_load)
    std::map<GaussKey, GaussTable> gauss;                    // gaussian kernel tables (gauss_tables.cpp)
    std::map<const GaussTable *, double *> gauss_dev;        // their device copies (stack_pipeline.cpp)
    hipStream_t stream = nullptr;
    int patch = 0, max_patches = 0;
    int f0 = 0, f_last = 0;
    float *stem_w = nullptr, *stem_scale = nullptr, *stem_shift = nullptr;
    std::vector<DownBlock> down;
    std::vector<UpBlock> up;
    float *final_w = nullptr;
    float final_b = 0.f;
    std::vector<void *> owned;              // weight allocations
    float *buf[4] = {nullptr, nullptr, nullptr, nullptr};    // down-path ping-pong activations
    float *ubuf[4] = {nullptr, nullptr, nullptr, nullptr};   // up-path activations
    float *dout[2] = {nullptr, nullptr};                     // down-path output (P/16)^2 x f_deep, double-buffered
    // activated copies (max(x, +0)) of the tensors a block's first convolution reads: the bottleneck (written by the last pooling) and
    // the outputs of up blocks 0 .. n-2 (written by conv_mfma_kernel's epilogue); TMAT_RELU_COPY=0: ReLU on load instead
    bool relu_copy = true;
    float *dout_relu[2] = {nullptr, nullptr};
    bool dout_relu_ok[2] = {false, false};                   // the last down-path call wrote dout_relu[i] (only the unfused last block does)
    float *urelu[2] = {nullptr, nullptr};
    hipStream_t stream2 = nullptr;                           // second stream: down path of pass p+1 overlaps up path of pass p
    hipStream_t stream3 = nullptr;                           // third stream: finish stage of pass p-1 (after the host thinning)
    hipEvent_t ev_down[2] = {nullptr, nullptr};
    hipEvent_t ev_pre[2] = {nullptr, nullptr};              // front end of a pass (Lanczos ... tile gather) done: patch_in_of(slot) is complete
    bool down_pending[2] = {false, false};
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_blend[2] = {nullptr, nullptr};      // the tail of a pass (blend, mask filter, EDT) on the second stream
    bool blend_pending[2] = {false, false};
    float *patch_in = nullptr, *patch_out = nullptr;
    float *patch_in2 = nullptr;                              // second input buffer of the batch path: the front end of pass p + 2 runs beside pass p + 1's network (pipeline.cpp)
    bool pre_side = true;                                    // that front end on the second stream (TMAT_PRE_STREAM=0: on the main stream)
    float input_sat = 65535.f;                               // Lanczos saturation: 65535, or 255 for 8-bit sources (tmat_set_input_depth)
    int patch_cap = 0;                                       // patches patch_in / patch_out hold (>= max_patches)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    // owns the handle-lifetime workspaces above: buf, ubuf, dout, dout_relu, urelu, patch_in, patch_in2, patch_out, scratch
    WsList ws;
    double *win1d = nullptr;
    std::vector<double> win_host;
    PassBuf pass;
    void free_pass()
    {
        PassBuf &b = pass;
        b.ws.free_all();
        void *lanczos[] = {b.xi, b.yi, b.xc, b.yc};
        for (void *p : lanczos) if (p) hipFree(p);
        for (hipEvent_t e : b.done) if (e) hipEventDestroy(e);
        pass = PassBuf();
    }
    bool thin_device = true;                                 // ordered medial-axis thinning on the device (TMAT_THIN_DEVICE=0: host threads)
    uint32_t *ma_table = nullptr;                            // its 512-entry decision table, 16 words
    double *se_table = nullptr;                              // candidate table of the superellipse search, [se_iters][7] (wellfit_kernels.hip): a constant, like ma_table
    int se_iters = 0;
    bool dmt_device = true;                                  // DMT key build + lower-star sort on the device (TMAT_DMT_DEVICE=0: host)
    bool dmt_sweep_device = true;                            // the two persistence sweeps on the device as well (TMAT_DMT_SWEEP_DEVICE=0: host threads)
    bool fused_pool = true;                                  // max-pool + residual add fused behind the second separable convolution (TMAT_FUSED_POOL=0: separate kernel)
    bool norm_on = false;                                    // models.py:636-637 input normalisation in front of the smooth prediction (tmat_set_input_norm)
    float norm_mean = 0.f, norm_std = 1.f;
    int resnet_precision = 0;                                // invasion-depth classifiers: TMAT_RESNET_PRECISION_F32 (bit-exact contract), _F16 or _F16ACT (opt-in, tmat_resnet_set_precision)
    bool narrow = false;                                     // some convolution of the model runs on the narrow kernel (conv_narrow_kernels.hip): f32 only
    int png_mode = 0;                                        // TMAT_PNG_FAST or TMAT_PNG_COMPACT (opt-in, tmat_png_set_mode): every PNG file this handle encodes
    int precision = 0;                                       // TMAT_PRECISION_F32 (bit-exact contract) or TMAT_PRECISION_BF16X3 / _BF16X6 (opt-in, tmat_set_precision)
    std::map<const float *, ConvWHost> conv_w_host;          // device pointer of every MFMA convolution weight tensor -> its host copy
    std::map<int, std::map<const float *, float *>> wsplit;  // precision mode -> (... -> its split-precision copy on the device, made on first use)
    bool sep_bf16 = true;                                    // bf16x3 mode also runs the separable layers' pointwise part on the bf16 cores (TMAT_SEP_BF16=0: f32)
    bool stem_fused = true;                                  // the stem recomputed inside block 0's first separable convolution (TMAT_STEM_FUSED=0: stem_kernel writes its tensor)
    // region form of the tiled up path (roi_plan.h): plans per image geometry, made on first use, with the device table of the class-major
    // patch order (TileGeom::order).  TMAT_ROI=0: whole patches in every layer, image-major order
    bool roi_on = true;
    // TMAT_ROI_TIGHT: the up path launches the tight rectangles (RoiPlan::rect_tight: every layer rounds its own need); 0: the nested ones
    bool roi_tight = true;
    // TMAT_ROI_EXACT: with the tight plan, a layer's rectangle is its need itself, columns unrounded (RoiPlan::rect_exact; the row-split
    // epilogue of conv_mfma_kernel<..., ROI> takes them); 0: the tight rectangles.  No effect without TMAT_ROI and TMAT_ROI_TIGHT
    bool roi_exact = true;
    // TMAT_ROI_DOWN: what of the down path the tiled entry points run in region form too (roi_plan.h:RoiDownPlan).  Bit 0: the unfused
    // level, the residual 1x1 layers, the stem at the even pixels, the pooling fix-ups.  Bit 1: the fused separable layers visit only
    // the tiles of their rectangles (RoiEntry::tabs).  0: the down path stays full-frame
    unsigned roi_down = 3u;
    // The four switches of the down path's forms above ROI_DOWN_REGION, each on top of the one before it (roi_plan.h:RoiDownForm).  All
    // are tri-state: -1 (unset): the batch pipeline runs the form, predict_smooth does not (tests pin its launches to the dependency
    // plan's tiles); 0: nobody; 1: both.  ONE place turns them, the plan and the pass into the form a pass runs: roi_down_resolve.
    // TMAT_ROI_CONST, ROI_DOWN_CONST (roi_plan.h:RoiDownPlan::live): what the padding ring makes constant is copied from an all-constant
    // patch per image instead of computed.  The k all-constant patches of a pass of k images ride behind its patches in the same
    // launches: the down-path workspaces and the input buffers hold const_cap patches more than max_patches, and a pass of more images
    // (fewer than 64 patches per image at the default size) keeps the dependency plan.
    int roi_const = -1;
    int const_cap = 0;
    // TMAT_ROI_SHARE, ROI_DOWN_SHARE (roi_plan.h:RoiDownPlan::share): what a patch's successor on an axis computes of their overlap is
    // copied, not computed again; the fused separable layers skip the tiles that leaves without a needed pixel.  Only where the
    // constant-ring form runs, and only with the tile tables (TMAT_ROI_DOWN bit 1).
    int roi_share = -1;
    // TMAT_ROI_SHARE_RECT, ROI_DOWN_SHARE_RECT (roi_plan.h:RoiDownPlan::rcomp): the rectangle launches of the unfused 40² level take the
    // shared-interior form too: several disjoint rectangles per class in their segment tables, the bottleneck tensor's shared zone
    // copied.  Only where the shared-interior form runs, and only with the rectangle launches (TMAT_ROI_DOWN bit 0).
    int roi_share_rect = -1;
    // TMAT_ROI_SHARE_FUSED_RECT, ROI_DOWN_SHARE_FUSED_RECT (roi_plan.h:RoiDownPlan::fcomp): the rectangle launches of the fused 160² and
    // 80² levels -- stem at the even pixels, stride-2 residual 1x1, pooling fix-up -- take the shared-interior form as well, and the
    // pooled outputs are copied as halo strips, not as whole zones.  Only where the rectangle launches' form of the unfused level runs:
    // while that level reads the pooled outputs whole, strips are not enough.
    int roi_share_fused_rect = -1;
    // TMAT_ROI_QUAD, the same tri-state: the plain fused layers 6 b + 1 of the levels in ROI_QUAD_LEVELS visit 8 x 8 quadrants, four to a
    // packed tile, instead of 16 x 16 tiles (roi_plan.h:roi_sep_quad_table).  No form of its own (the rectangles, copies and the pooled
    // layers' tiles are those of the resolved form): a property of those launches where the shared-interior form or one above it runs.
    int roi_quad = -1;
    // TMAT_ROI_QUAD_POOL, the same tri-state and independent of TMAT_ROI_QUAD: the pooled fused layers 6 b + 3 of the levels in
    // ROI_QUAD_POOL_LEVELS visit quadrants too (roi_plan.h:roi_sep_quad_pool_table), their strips are kept per quadrant and the pooling
    // fix-up behind them finishes the quadrant edges.  The strips live in buf[3], which holds a whole second-layer tensor per patch: 36
    // strip pixels per 256-pixel tile (17 in the tile form) fit with room to spare, so the handle holds the same bytes under every setting.
    int roi_quad_pool = -1;
    float *padval[2] = {nullptr, nullptr};                   // the pad values of a pipeline pass, per slot: c->scratch is rewritten by the front end of the pass after next
    std::vector<RoiEntry *> roi_cache;
    std::vector<std::pair<long long, long long>> sep_tiles;  // (planned, full) tiles of the fused separable launches of the last down pass (tmat_debug_sep_tiles)
    int down_segs = 0;                                       // the longest segment table of the last down pass's launches (tmat_debug_down_segs)
    int down_seg_total = 0;                                  // the segments of all its rectangle launches together (tmat_debug_down_seg_total)
    bool fused_sep = true;                                   // fused depthwise -> pointwise kernel (sepconv_ws_kernel) where the level allows (TMAT_FUSED_SEP=0: separate kernels)
    // call-scoped device workspaces of the side tools (cell area, invasion depth), kept between calls: with the reference's default batch of 4 images a
    // hipMalloc / hipFree pair per buffer and call costs more than the batch's kernels.  Slot = a ToolWs id per buffer (ws_get below).
    void *tool_ws[N_TOOL_WS] = {};
    size_t tool_ws_bytes[N_TOOL_WS] = {};
    WsPool ws_pool;                                          // released call-scoped blocks of the Z-stack tool, by size (dev_mem.h:DevScope::pooled)
    WsList stack_host;                                       // pinned result buffers of the Z-stack batch pipeline, two slots of five (stack_pipeline.cpp)
    std::vector<std::pair<double, double>> stack_trace;      // (device stages ms, host graph stage ms) per pass of the last tmat_analyze_stack_batch
    // profiling of the dominant kernel family
    bool prof_on = false;
    std::vector<ProfEv> ev_open;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms = 0, prof_flops = 0;
    int64_t prof_launches = 0;
};

int unet_forward_dev(Ctx *c, const float *X, int n, float *Y, hipStream_t s);
int ensure_patch_io(Ctx *c, int n_patches);
// The form a down pass of kimg images runs (roi_plan.h:RoiDownForm): the highest one that the handle's switches ask for -- by_default:
// the entry point runs a form whose switch is unset (the batch pipeline does, predict_smooth does not) --, that the handle and the
// pass allow and that the plan has.  have_padval: the pad values of the pass's images are on the device.  The one place where the
// eligibility chain is written down; both tiled entry points go through it.
RoiDownForm roi_down_resolve(const Ctx *c, const RoiPlan *plan, int kimg, bool have_padval, bool by_default);
// plan + form (tiled callers): n is a whole number of images' patches in the plan's class-major order and form what roi_down_resolve
// gave for the pass.  padval: the pad values of the pass's images on the device, from ROI_DOWN_CONST upwards.  X then has room for
// n + n / tiles_per_img patches (patch_in and patch_in2 do): the all-constant patches are written there
// quad: roi_quad_on of the entry point -- from ROI_DOWN_SHARE upwards the plain fused layers take their quadrant tables
// quad_pool: roi_quad_pool_on of the entry point -- the same for the pooled fused layers and their fix-up launches
int unet_down_dev(Ctx *c, const float *X, int n, float *dout, hipStream_t s, const RoiPlan *plan = nullptr, const float *padval = nullptr,
                  RoiDownForm form = ROI_DOWN_FULL, bool quad = false, bool quad_pool = false);
inline bool roi_quad_on(const Ctx *c, bool by_default) { return by_default ? c->roi_quad != 0 : c->roi_quad == 1; }
inline bool roi_quad_pool_on(const Ctx *c, bool by_default) { return by_default ? c->roi_quad_pool != 0 : c->roi_quad_pool == 1; }
// plan (nullable): region form; n is then a whole number of images' patches in the plan's class-major order
int unet_up_dev(Ctx *c, const float *dout, int n, float *Y, hipStream_t s, const RoiPlan *plan = nullptr);
// the region plan of g's geometry (cached on the handle) and, in g.order, its patch order; null and the image-major order when the region
// form is off, the image needs more patches than the workspace holds, or it has more classes than a launch carries
const RoiPlan *roi_attach(Ctx *c, TileGeom &g);
const RoiPlan *roi_find(const Ctx *c, const TileGeom &g);
int predict_smooth_dev(Ctx *c, float *x_dev, int n, int hh, int ww, double *pred_dev);      // x_dev is normalised in place when tmat_set_input_norm is on

// squared-spline window of smooth_tiled_predictions.py:26-41 for any ws >= 4 (scipy's triang in its even and odd forms, numpy's mean)
std::vector<double> spline_window_host(int ws);

// numpy's pairwise summation of a contiguous f64 vector (np.add.reduce / np.mean inner loop):
// 8 interleaved partial sums on blocks <= 128, recursive halves (rounded down to a multiple of 8) above.
inline double numpy_pairwise_sum(const double *a, long n)
{
    if (n < 8) {
        double res = 0.0;
        for (long i = 0; i < n; i++) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; j++) r[j] = a[j];
        long i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    long n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_pairwise_sum(a, n2) + numpy_pairwise_sum(a + n2, n - n2);
}

// device workspace `slot` of the handle with room for `bytes` (grown by reallocation: the caller's stream must not have work in flight on
// the old buffer -- every user synchronises before it returns); nullptr + set_error on failure
inline void *ws_get(Ctx *c, ToolWs slot, size_t bytes)
{
    if (c->tool_ws_bytes[slot] >= bytes && c->tool_ws[slot]) return c->tool_ws[slot];
    if (c->tool_ws[slot]) { hipFree(c->tool_ws[slot]); c->tool_ws[slot] = nullptr; c->tool_ws_bytes[slot] = 0; }
    if (!hip_ok(hipMalloc(&c->tool_ws[slot], bytes ? bytes : 16), "hipMalloc(tool workspace)")) { c->tool_ws[slot] = nullptr; return nullptr; }
    c->tool_ws_bytes[slot] = bytes ? bytes : 16;
    return c->tool_ws[slot];
}

// TMAT_INV_DEPTH_PRECISION=f32|f16|f16act at handle creation (resnet_kernels.hip): TMAT_OK, or TMAT_E_ARG with the error set for any other value
int resnet_precision_from_env(Ctx *c);

// handles made by tmat_create_plain carry no model
inline bool has_model(const Ctx *c) { return c && !c->up.empty(); }
}  // namespace tmat
