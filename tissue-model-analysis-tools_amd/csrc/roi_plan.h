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

struct RoiRect { int y0, x0, rh, rw; };

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
    double mac_planned[ROI_MAX_LAYERS] = {}, mac_full[ROI_MAX_LAYERS] = {};      // multiply-accumulates per image
};

// chan[0]: input channels of up block 0, chan[j + 1]: output channels of up block j (n_up + 1 entries)
bool roi_make_plan(int hh, int ww, int ws, int n_up, const int *chan, int max_classes, RoiPlan &out);

}  // namespace tmat
