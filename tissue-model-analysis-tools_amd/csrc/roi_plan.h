// Region planner of the UNet up path (host only, no GPU needed): which pixels of every up-path tensor the blend can reach.
//
// predict_img_with_smooth_windowing pads the image by aug = ws / 2, tiles the padded frame and throws the padding ring away after
// the blend (blend_kernels.hip:blend_kernel only gathers at pixels (yo + aug, xo + aug) inside the image).  Of a patch (g, a, b) the
// blend therefore reads the rectangle  patch ∩ interior  only (frame coordinates of orientation g; the ring is symmetric, so the
// interior is [aug, F - aug) on both axes of every orientation).  The up path has no long skip connections: the rectangle is walked
// backwards layer by layer (final conv, then per block: second 3x3 + low-resolution residual, first 3x3 / sub-pixel, residual 1x1),
// every producer's rectangle being the hull of its consumers' rectangles dilated by their tap reach, clipped to the patch and rounded
// OUTWARDS to the form conv_mfma_kernel likes (a superset only costs time).  Patches with the same rectangle form a CLASS; within a
// pass the patches are stored class-major, so that a class is a contiguous patch range and a launch needs one segment per class.
#pragma once
#include <vector>

namespace tmat {

constexpr int ROI_MAX_CLASSES = 16;
constexpr int ROI_MAX_UP = 5;
constexpr int ROI_MAX_LAYERS = 3 * ROI_MAX_UP + 1;
constexpr int ROI_MAX_DOWN = 4;
constexpr int ROI_MAX_DOWN_LAYERS = 6 * ROI_MAX_DOWN + 4;

struct RoiRect { int y0, x0, rh, rw; };
struct RoiSegs;
struct FillItems;
struct ShareItem;

// Layers of the up plan (bit l: layer l) whose EXACT rectangle is their tight one: none.  (The place for a layer that a per-launch trace
// shows slower with unrounded columns than with rounded ones; DESIGN 4.1.1 has the trace.)
constexpr unsigned ROI_EXACT_KEEP_TIGHT = 0u;

// The same walk continued through the down path (roi_plan_down), from what up block 0 reads of the bottleneck tensor to the input window.
// Layer 6 b + k belongs to down block b (input side (ws / 2) >> b): k = 0 first depthwise, 1 first pointwise, 2 second depthwise,
// 3 second pointwise (all at the block's input resolution), 4 the stride-2 residual 1x1, 5 max-pool + add (both enumerate OUTPUT pixels,
// half the side).  Then 6 n_down: the stem at its even pixels (side ws / 4: the residual's input when the stem lives inside the first
// separable layer), 6 n_down + 1: the stem (side ws / 2), 6 n_down + 2: the input window (side ws), 6 n_down + 3: the rectangle of the
// network's output that the blend reads (side ws), where the walk starts.
// need: the pixels the blend depends on, exactly, each from its consumers' NEED dilated by their taps (MaxPooling2D(3, 2, "same") on an
// even side reads 2 i .. 2 i + 2, the stem likewise; a depthwise layer one pixel around; the residual the even pixels).  rect: what the
// layer's kernel computes, need rounded outwards: whole 16 x 16 tiles on the fused separable kernel (a level in fused_mask), the column
// rule of conv_mfma_kernel<..., ROI> for the pointwise and residual layers and the depthwise strips in front of them, single pixels for
// the pooling.  A pixel of rect outside need may be computed from operands nobody wrote; nothing needed depends on it.
struct RoiDownPlan {
    struct ShareFill { int layer, cls, dir, y0, x0, rh, rw; };     // a copy out of a neighbour patch: see share_fill
    int n_down = 0, n_layers = 0;               // 6 n_down + 4; 0: no down plan
    unsigned fused_mask = 0;
    int res[ROI_MAX_DOWN_LAYERS] = {};
    RoiRect need[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {}, rect[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {};
    // per image: multiply-accumulates of the matrix work (pointwise and residual layers), bytes moved by the kernels without any
    // (unfused depthwise, pooling, stem at the even pixels)
    double mac_planned[ROI_MAX_DOWN_LAYERS] = {}, mac_full[ROI_MAX_DOWN_LAYERS] = {};
    double bytes_planned[ROI_MAX_DOWN_LAYERS] = {}, bytes_full[ROI_MAX_DOWN_LAYERS] = {};
    bool free_tile[ROI_MAX_DOWN] = {};          // fused level b: some class skips a whole 16 x 16 tile of either separable layer

    // The CONSTANT-RING form (TMAT_ROI_CONST).  A patch is image data inside read[c] and one value per image (the pad value) outside.
    // nonconst: the pixels whose receptive field, clipped to the patch, reaches read[c] -- the forward walk from the input window through
    // the taps the backward walk uses (roi_plan.cpp:TAP_*).  Outside it a tensor equals, bit for bit, the same tensor of a patch that is
    // the pad value everywhere, at the same position (not one vector per layer: SAME pads zeros, the borders differ).
    // live: what a launch still has to compute, need ∩ nonconst.  A tensor that is never stored (the depthwise outputs and the second
    // pointwise output of a fused level, the stem inside the STEM layer) cannot be copied: its live is the taps of its consumer's live.
    // rect_live: live rounded outwards by rect's rule, inside rect.
    // fill: the pixels of a STORED tensor outside nonconst that a consumer's live reads through its taps (for the bottleneck tensor:
    // that up block 0 reads), as at most four strips -- above, below, left and right of nonconst.  The launches copy them from the
    // all-constant patch of the image.  Every tap of a consumer's live lies in the producer's live ∪ fill.
    RoiRect nonconst[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {}, live[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {};
    RoiRect rect_live[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {};
    RoiRect fill[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES][4] = {};
    bool stored[ROI_MAX_DOWN_LAYERS] = {};      // the layer's output is a tensor in memory that a region-form launch writes
    double mac_live[ROI_MAX_DOWN_LAYERS] = {}, bytes_live[ROI_MAX_DOWN_LAYERS] = {};       // mac_planned / bytes_planned of rect_live

    // The SHARED-INTERIOR form (TMAT_ROI_SHARE), on top of the constant-ring form.  The patches of an orientation overlap by half a
    // side: position v of a tensor of side H is position v - H / 2 of the next patch on that axis.  Both patches hold the same bits
    // there unless the position's receptive field crosses either patch's border, where SAME pads zeros.  All sets are per AXIS and
    // depend on the axis KEY only -- the interval of `read` on that axis -- so that patches in one row (column) of the grid agree on
    // their row (column) sets; a class's 2-D set is the product.
    // inner: the complement of the RING, the outputs whose receptive field, clipped to the patch, touches the patch border -- the
    // forward walk from both borders through the taps of walk_const_axis (TAP_S2 pads at the far end only).
    // share (rows [0..1], columns [2..3] as lo, hi): positions v in live and inner whose v - H / 2 is, in EVERY patch that follows a
    // patch of this key on either axis anywhere, inner and computed by that patch itself; empty when some patch of the key has no
    // successor.  Only the stored tensors of the fused levels in ROI_SHARE_LEVELS have one: the first layer's output (6 b + 1) and the
    // pooled output (6 b + 5).
    // comp ([layer][class][axis][ws] bytes, the first res[layer] used): the NEEDED pixels the patch computes itself -- live \ share for
    // the pooled output, and backwards from there through the taps for the fused layers; live everywhere else (rectangle launches keep
    // rect_live).  The fused layers run the tiles that hold a comp pixel (roi_sep_tile_table: tile_rows x tile_cols, bit t).
    // share_fill: the pixels in share that a consumer's comp taps -- of 6 b + 1 the halo strips of the pooled layer's tiles, except
    // where they lie in a tile of 6 b + 1 that runs anyway (they join comp: the block's input is held whole; at the network's sizes
    // that is all of them), of 6 b + 5 all of share (the next level's rectangle launches read the tensor whole) -- as rectangles
    // with a direction: copied from the
    // right (0), lower (1) or diagonal (2) neighbour at (y, x - S), (y - S, x), (y - S, x - S).  Every source pixel is in its own
    // patch's comp.  Every tap of a comp pixel lies in the producer's comp ∪ fill ∪ share_fill.
    bool share_any = false;                     // some class shares: the form differs from the constant-ring form
    RoiRect inner[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {};
    int share[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES][4] = {};
    unsigned long long tile_rows[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {}, tile_cols[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {};
    std::vector<unsigned char> comp;
    std::vector<ShareFill> share_fill;
    std::vector<int> nbr;                       // [tiles_per_img][3]: the image-major tile right of, below and diagonally below a tile, or -1

    // The shared-interior form of RECTANGLE launches comes twice, one on top of the other, and both times as one RectForm, built like
    // share / comp, per axis and axis key, in fields of its own: everything above keeps its values.
    //   mask (layout of comp): the exact sets in force under the form, every layer.
    //   rects[l][k][0 .. n[l][k]): the rectangles layer l launches for class k under the form: at most four, disjoint, inside rect_live,
    //   and they hold the exact set.  Rows exact; columns as the form says.  A rectangle that rounding or whole tiles add on top of an
    //   exact set may read words nobody wrote: the contract of rect.
    //   fill: the copies out of the neighbour patches that the form adds, same directions and same source rule as share_fill.
    //   any false: the plan has no such form -- every field but mask is then the copy of the form below (of rect_live for rcomp).
    struct RectForm {
        bool any = false;                       // some class's rectangles or some copy list differ from the form below
        int n[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES] = {};
        RoiRect rects[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES][4] = {};
        std::vector<unsigned char> mask;
        std::vector<ShareFill> fill;
        // mac_planned / bytes_planned of rects, and their pixels per image
        double mac[ROI_MAX_DOWN_LAYERS] = {}, bytes[ROI_MAX_DOWN_LAYERS] = {}, px[ROI_MAX_DOWN_LAYERS] = {};
        int segs = 0;                           // the longest segment table a launch of the form needs (without the constant patches' segment)
    };
    // rcomp, ROI_DOWN_SHARE_RECT (TMAT_ROI_SHARE_RECT), on top of the shared-interior form: the last level, where it is unfused and in
    // ROI_SHARE_RECT_LEVELS (layers 6 b + 0 .. 6 b + 5, b = n_down - 1: the 40² level of the network).
    // rshare (row lo, row hi, column lo, column hi): the zone of the bottleneck tensor 6 b + 5, same rule as share.  It is the only
    // tensor of the level that is copied: all of rshare (it lies in live, which is what up block 0 reads), into the tensor and into
    // its activated copy -- rcomp.fill.
    // rcomp.mask: live \ rshare for 6 b + 5, and backwards from there through the taps, inside live, for 6 b + 4 .. 6 b:
    // the halo of a consumer's comp (1 pixel per side under a depthwise layer, 2 i .. 2 i + 2 under the pooling) JOINS comp, so no
    // intermediate tensor needs a copy (DESIGN 4.1.5 has the pixels against the bytes).  Per axis comp is live minus one interval: at
    // most two runs, and a class's 2-D set at most four disjoint rectangles.  Every other layer: live.
    // rcomp.rects: the columns of layers 6 b + 0 .. 6 b + 4 rounded outwards to multiples of 4 inside rect_live (a rounded rectangle may
    // reach into the shared gap: a superset only costs time; two runs that meet after rounding are one).  Every other layer, and every
    // class that shares nothing: rect_live itself.
    int rshare[ROI_MAX_DOWN_LAYERS][ROI_MAX_CLASSES][4] = {};
    RectForm rcomp;
    // fcomp, ROI_DOWN_SHARE_FUSED_RECT (TMAT_ROI_SHARE_FUSED_RECT), on top of both forms above: the rectangle launches of the FUSED
    // levels -- the stride-2 residual 1x1 (6 b + 4) and the pooling fix-up (6 b + 5) of a fused level b in ROI_SHARE_FUSED_RECT_LEVELS,
    // and the stem at the even pixels (6 n_down) with level 0.  The form exists only where rcomp.any holds: while the unfused level
    // reads the pooled outputs whole, their whole zone has to be copied.
    // fcomp.mask: comp of the pooled output 6 b + 5 (live \ share) as it is; the residual 6 b + 4 that set cut by its own live; the stem
    // at the even pixels block 0's residual set cut by its own live; rcomp.mask for the unfused last level; comp for every other layer.
    // A class takes the form in all rectangle launches of a level or in none (its keys share at the level and every set lies inside
    // its rect_live).
    // fcomp.rects (rcomp.rects for every layer outside the form): the columns of the residual and stem layers rounded outwards to
    // multiples of 4 inside rect_live (two runs that meet after rounding are one), the pooled layer in single pixels.
    // fcomp.fill: the copies of a pooled output 6 b + 5 as HALO STRIPS, in place of its items in share_fill (fused_fill_on[6 b + 5]):
    // only the shared pixels that a consumer's exact set taps in the next level -- the depthwise taps of fcomp.mask[6 (b + 1)], the even
    // pixels under fcomp.mask[6 (b + 1) + 4] -- per axis, the 2-D list being the product (a superset of both consumers' products).
    // A table that does not fit a launch's segments keeps the form below.
    bool fused_fill_on[ROI_MAX_DOWN_LAYERS] = {};
    RectForm fcomp;
    double px_live[ROI_MAX_DOWN_LAYERS] = {};                                              // pixels per image of rect_live
    double copy_old[ROI_MAX_DOWN_LAYERS] = {}, copy_new[ROI_MAX_DOWN_LAYERS] = {};         // pixels per image copied into the tensor: share_fill, under fcomp
};

// The forms of the down path, each on top of the one before it.  A pass runs ONE of them (tmat_api.cpp:roi_down_resolve), and what a
// layer launches under a form is answered here, by roi_down_segs (roi_down_rects, roi_down_stem_layer), roi_sep_tile_table,
// roi_down_const_items and roi_down_copy_items -- for the launches and for tmat_roi_down_schedule alike.
//   ROI_DOWN_FULL              whole patches everywhere: no segment table, no tile table, no copy
//   ROI_DOWN_REGION            rect; the fused separable layers the tiles of rect
//   ROI_DOWN_CONST             rect_live, the tiles of rect_live; every stored tensor takes the strips of `fill` from the constant patches
//   ROI_DOWN_SHARE             the tiles of tile_rows x tile_cols; the stored tensors of the fused levels take share_fill after `fill`
//   ROI_DOWN_SHARE_RECT        rcomp.rects; the bottleneck tensor (and its activated copy) takes rcomp.fill
//   ROI_DOWN_SHARE_FUSED_RECT  fcomp.rects, the stem at the even pixels its own layer's; a pooled output in fused_fill_on takes its items
//                              of fcomp.fill in place of its items of share_fill
// The copies of a stored tensor, after the launch that writes it and before its first reader, in this order: the constant strips from
// ROI_DOWN_CONST upwards; then the neighbour items -- the layer's items of share_fill, or of fcomp.fill in their place where
// fused_fill_on[layer], and the layer's items of rcomp.fill (share_fill has items on fused levels only, rcomp.fill on the unfused last
// level only: a layer has items in one of them at most).
enum RoiDownForm { ROI_DOWN_FULL, ROI_DOWN_REGION, ROI_DOWN_CONST, ROI_DOWN_SHARE, ROI_DOWN_SHARE_RECT, ROI_DOWN_SHARE_FUSED_RECT };

// Fused levels (bit b) that take the shared-interior form: a level whose copies cost more than its skipped tiles save is taken out here
constexpr unsigned ROI_SHARE_LEVELS = 3u;
// Levels (bit b) whose rectangle launches take it too (RoiDownPlan::rcomp).  Built for the last level where it is unfused -- bit 2, the
// 40² level; the rectangle launches of the fused levels (bits 0 and 1) have a form of their own, below
constexpr unsigned ROI_SHARE_RECT_LEVELS = 4u;
// Fused levels (bit b) whose rectangle launches -- stride-2 residual, pooling fix-up, with bit 0 the stem at the even pixels -- take the
// shared-interior form (RoiDownPlan::fcomp) and whose pooled output is copied as halo strips.  A level whose form does not pay is taken
// out here, by one bit
constexpr unsigned ROI_SHARE_FUSED_RECT_LEVELS = 3u;
// Fused levels (bit b) whose plain layer 6 b + 1 visits 8 x 8 quadrants instead of 16 x 16 tiles (roi_sep_quad_table) where a pass runs
// the quadrant form (TMAT_ROI_QUAD).  A level whose launch does not pay is taken out here, by one bit; it keeps its tile table
constexpr unsigned ROI_QUAD_LEVELS = 3u;
// The same for the pooled layer 6 b + 3 (roi_sep_quad_pool_table; TMAT_ROI_QUAD_POOL): its launch and the pooling fix-up behind it then
// work in quadrants.  Set by the per-launch trace of DESIGN 4.1.9
constexpr unsigned ROI_QUAD_POOL_LEVELS = 3u;

struct RoiPlan {
    int hh = 0, ww = 0, ws = 0, n_up = 0;
    int tiles_per_img = 0;
    int n_classes = 0;                          // 0: no plan (more classes than the cap): every launch stays full-frame, patches image-major
    int n_layers = 0;                           // 3 n_up + 1
    // class-major patch order of a pass of k images: patch (img, tile) lives at  k class_base[c] + img class_count[c] + tile_rank[tile],
    // c = tile_class[tile]  (tile = the image-major index tile_off[g] + a nb + b of blend_kernels.hip)
    int class_base[ROI_MAX_CLASSES + 1] = {};
    int class_count[ROI_MAX_CLASSES] = {};
    std::vector<int> tile_class, tile_rank;     // [tiles_per_img]
    // layer 3 j: first convolution of up block j (3x3 at j = 0; sub-pixel form above: the rectangle enumerates STORED pixels),
    // 3 j + 1: its residual 1x1, 3 j + 2: its second 3x3, 3 n_up: the final convolution (stored pixels; whole 8 x 16 blocks of final_kernel)
    int res[ROI_MAX_LAYERS] = {};               // side of the square a layer enumerates
    RoiRect rect[ROI_MAX_LAYERS][ROI_MAX_CLASSES] = {};
    // The TIGHT rectangles of the same layers and classes, what the tiled entry points launch by default.  rect above is NESTED: a
    // producer covers its consumer's ROUNDED rectangle plus the taps, and rounds again, so the columns drift outwards layer after layer.
    // Here a layer's rectangle is its own need -- the exact dependency closure of `read`, walk_back(..., exact) -- with the columns rounded
    // outwards once by the same rule (rows exact; the final convolution keeps rect's whole 8 x 16 blocks).  The contract is the down
    // plan's: a pixel of a rectangle outside the need may be computed from operands nobody wrote (the kernels address every tensor by
    // full-frame position, so such a read lands on an in-bounds word of the workspace), and nothing needed depends on it.
    // rect_tight[l][k] lies inside rect[l][k].
    RoiRect rect_tight[ROI_MAX_LAYERS][ROI_MAX_CLASSES] = {};
    // The EXACT rectangles: a layer's rectangle IS its need, rows and columns (walk_back(..., exact, parity): the bounding box of the pixels
    // the blend depends on, the sub-pixel layers' reads following the parity of their outputs), no rounding at all -- odd first
    // columns and odd widths are the normal case; conv_mfma_kernel<..., ROI>'s per-lane prologue and row-split epilogue take them (a group
    // of consecutive pixels may break into the next row once).  The final convolution keeps rect's whole 8 x 16 blocks.  A layer in
    // ROI_EXACT_KEEP_TIGHT keeps its tight rectangle.  rect_exact[l][k] lies inside rect_tight[l][k]; the contract is the same.
    RoiRect rect_exact[ROI_MAX_LAYERS][ROI_MAX_CLASSES] = {};
    // which set up_rects() names: set by the caller that launches (TMAT_ROI_TIGHT, TMAT_ROI_EXACT, tmat_api.cpp:roi_attach); exact has
    // effect only with tight
    bool tight = false, exact = false;
    const RoiRect *up_rects(int l) const { return tight ? (exact ? rect_exact[l] : rect_tight[l]) : rect[l]; }
    RoiRect read[ROI_MAX_CLASSES] = {};         // patch ∩ interior: the output pixels the blend reads of a patch of the class
    double mac_planned[ROI_MAX_LAYERS] = {}, mac_full[ROI_MAX_LAYERS] = {};      // multiply-accumulates per image
    double mac_planned_tight[ROI_MAX_LAYERS] = {};                               // the same of rect_tight
    double mac_planned_exact[ROI_MAX_LAYERS] = {};                               // the same of rect_exact
    RoiDownPlan down;                           // filled by roi_plan_down
};

// chan[0]: input channels of up block 0, chan[j + 1]: output channels of up block j (n_up + 1 entries)
bool roi_make_plan(int hh, int ww, int ws, int n_up, const int *chan, int max_classes, RoiPlan &out);
// chan[0]: channels of the stem, chan[b + 1]: output channels of down block b (n_down + 1 entries); fused_mask bit b: block b runs on the
// tile-granular fused separable kernel (bit 0 then also means: the stem is recomputed inside the first separable layer).  Needs a plan
// with classes; false (p.down left empty) otherwise or on a geometry the down path's kernels do not take.
bool roi_plan_down(RoiPlan &p, int n_down, const int *chan, unsigned fused_mask);
// Fills the shared-interior tables of a plan with a down plan (called by roi_plan_down; p.down.share_any stays false where nothing is shared)
void roi_plan_share(RoiPlan &p);

// ---- what a pass launches under a form (the table at RoiDownForm) ----
// The form the plan runs where `want` is asked for: the highest form not above `want` that the plan has, and every form below it with
// it -- ROI_DOWN_FULL without a down plan, no sharing form where no class shares (share_any), neither rectangle form where its `any`
// is false or its longest table, with the constant patches' segment, does not fit a launch (ROI_MAX_SEGS).  Every accessor below
// resolves its form through this, so each falls back to the form below exactly where the plan has nothing of its own.
RoiDownForm roi_down_form(const RoiPlan &p, RoiDownForm want);
// The rectangles layer l launches for class k: rect under ROI_DOWN_REGION, rect_live under ROI_DOWN_CONST and ROI_DOWN_SHARE, rcomp's
// under ROI_DOWN_SHARE_RECT, fcomp's under ROI_DOWN_SHARE_FUSED_RECT -- at most four, disjoint, the empty ones left out.  Returns
// their count (0 under ROI_DOWN_FULL: the launch has no segment table).
int roi_down_rects(const RoiPlan &p, RoiDownForm form, int l, int k, RoiRect out[4]);
// The layer whose rectangles the stem at the even pixels launches: its own (6 n_down) under ROI_DOWN_SHARE_FUSED_RECT, block 0's
// residual 1x1 (4) otherwise -- below that form the two layers have the same rectangles
int roi_down_stem_layer(const RoiPlan &p, RoiDownForm form);
// The tiles a fused separable layer of the down plan visits in a pass of k images (layer = 6 b + 1 or 6 b + 3 of a level in fused_mask):
// full-frame tile ids  patch * TPP + ty * TW + tx  (TW = res / 16 tiles per row, TPP = TW * TW per patch), the patches in the pass's
// class-major order (class c holds the patches k class_base[c] .. k class_base[c + 1] - 1), row-major inside the class's rectangle of
// whole tiles.  The table depends on k: a shorter last pass has its own.  Under ROI_DOWN_REGION the tiles of rect; under
// ROI_DOWN_CONST those of rect_live, a subsequence of that table; from ROI_DOWN_SHARE upwards those of tile_rows x tile_cols inside
// rect_live, a subsequence of the live table in its order.  Returns the full-frame tile count k tiles_per_img TPP, 0 when the layer has
// no tile rectangles (or under ROI_DOWN_FULL); out.size() == that count means every patch is computed whole.
long long roi_sep_tile_table(const RoiPlan &p, RoiDownForm form, int layer, int k, std::vector<int> &out);
// The same launch at 8 x 8 QUADRANT granularity, for the plain fused layer 6 b + 1 from ROI_DOWN_SHARE upwards only (the pooled layer
// 6 b + 3 has a table of its own, below).  Walks the tiles of
// roi_sep_tile_table in their order and emits, per tile in slot order (qy, qx) row-major, the full-frame id
// patch * QW * QW + (2 ty + qy) * QW + 2 tx + qx  (QW = res / 8) of every quadrant that holds a comp pixel; then all four quadrants of
// every tile of the k all-constant patches behind the pass's patches.  The kernel takes the ids four to a packed tile, so the last
// group is padded by repeating its last id (the duplicate computes and writes the same bits): out.size() is a multiple of 4.
// *n_own: the ids of the pass's own patches, *n_ids: all ids before the padding.  Returns the full-frame tile count of the pass's own
// patches like roi_sep_tile_table, 0 (out empty) for any other layer or form.
long long roi_sep_quad_table(const RoiPlan &p, RoiDownForm form, int layer, int k, std::vector<int> &out, long long *n_own, long long *n_ids);
// The quadrant table of the POOLED fused layer 6 b + 3, from ROI_DOWN_SHARE upwards: the same rule, order, constant patches and padding
// on the layer's own comp (the 3 x 3 windows of the pooled pixels the patch computes itself: comp of 6 b + 5 through the pooling's taps).
// So for every pooled pixel a later launch or copy reads, every quadrant that holds a pixel of its window inside the patch is listed --
// what the tile table guarantees one level coarser: the launch leaves a quadrant's last pooled row and column as partial maxima and
// the fix-up pass completes them from the strips of the quadrants below and to the right.  0 (out empty) for any other layer or form.
long long roi_sep_quad_pool_table(const RoiPlan &p, RoiDownForm form, int layer, int k, std::vector<int> &out, long long *n_own, long long *n_ids);
// The launch arguments of layer l in a pass of k images (tmat_internal.h has the structs), in the pass's class-major patch order: class
// c holds the patches k class_base[c] .. k class_base[c + 1] - 1, classes without patches are left out, and the k all-constant
// patches of ROI_DOWN_CONST and above sit behind them, at k tiles_per_img.
// roi_down_segs: the segment table -- per class the rectangles of roi_down_rects, then, from ROI_DOWN_CONST upwards, one segment of whole
// patches for the constant patches (p0 .. rw filled; no segment under ROI_DOWN_FULL: the launch is full-frame).
// roi_down_const_items: the strips of RoiDownPlan::fill the layer's tensor takes from the constant patches; none below ROI_DOWN_CONST.
// roi_down_copy_items: the neighbour items it takes after them, by the rule at RoiDownForm; none below ROI_DOWN_SHARE.
void roi_down_segs(const RoiPlan &p, RoiDownForm form, int l, int k, RoiSegs &out);
void roi_down_const_items(const RoiPlan &p, RoiDownForm form, int l, int k, FillItems &out);
void roi_down_copy_items(const RoiPlan &p, RoiDownForm form, int l, int k, std::vector<ShareItem> &out);
// nbr in the class-major order of a pass of k images: [k tiles_per_img][3] positions, or -1
void roi_share_neighbours(const RoiPlan &p, int k, std::vector<int> &out);

}  // namespace tmat
