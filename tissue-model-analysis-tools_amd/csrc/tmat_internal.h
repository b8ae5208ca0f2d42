// Internal declarations shared by the translation units of libtmat_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace tmat {

void set_error(const std::string &msg);
bool hip_ok(hipError_t e, const char *what);
#define TMAT_HIP(call) do { if (!::tmat::hip_ok((call), #call)) return TMAT_E_HIP; } while (0)

// ---- UNet layer launchers (unet_kernels.hip); all tensors NHWC f32 on device ----------------
struct ConvArgs {
    const float *in;      // stored tensor (N, h, w, Cin)
    int N, h, w, Cin;
    int relu_in;          // relu applied on load
    int ksize;            // 1 or 3; 2 = sub-pixel form of a 3x3 over the 2x nearest-upsampled stored tensor (out is 2h x 2w)
    int stride;           // 1, or 2 with ksize 1 (TF SAME 1x1 s2 samples even indices)
    const float *W;       // [ksize*ksize][Cout][Cin] (k contiguous); ksize 2: [4 parity classes][4][Cout][Cin]
    int Cout;
    const float *scale;   // nullable: v = scale ? fmaf(acc, scale, shift) : acc + shift
    const float *shift;
    const float *resid;   // nullable: v += resid[n][y >> rs][x >> rs][co]
    int rs;
    int relu_out;
    float *out;           // (N, h/stride, w/stride, Cout); ksize 2: (N, 2h, 2w, Cout)
    float *out_relu;      // nullable (ksize 1 / 3 only): a second, activated copy max(v, +0) of the output -- for a consumer that would otherwise apply ReLU on load
    int prec;             // 0: f32 MFMA (bit-exact contract); 1 / 2: bf16x3 / bf16x6 split precision, W then points to the split copy of the weights;
                          // 3: f16 operands, one product (ksize 1 / 3 only), W points to the f16 plane of the weights
};
// Region form of a launch (the tiled up path, roi_plan.h): the patches [p0, p0 + np) compute the rectangle (y0, x0, rh, rw) of their
// output only (sub-pixel form and final convolution: of their STORED pixels).  The caller fills p0 .. rw of the non-empty segments, in
// ascending patch order; launch_conv fills the rest for its tile size.
struct RoiSeg {
    int p0, np, y0, x0, rh, rw;
    int mt0, M;                      // first M tile of the segment; its pixels np rh rw
    unsigned dhw_mul; int dhw_sh;    // exact division by rh rw and by rw (unet_kernels.hip:FastDiv)
    unsigned dw_mul; int dw_sh;
};
// Several segments may name the SAME patch range with disjoint rectangles (the rectangle launches' shared-interior form,
// roi_plan.h:RoiDownPlan::rcomp: up to four per class); patch ranges never descend and never overlap otherwise.
constexpr int ROI_MAX_SEGS = 64;         // 4 per class over 15 classes, the constant patches' segment, room to spare: 3 KB of the 4 KB of kernel arguments
struct RoiSegs {
    int nseg;
    RoiSeg s[ROI_MAX_SEGS];
    long long pixels() const { long long t = 0; for (int i = 0; i < nseg; i++) t += (long long)s[i].np * s[i].rh * s[i].rw; return t; }
};
// The kernels without matrix work (depthwise, pooling, stem at the even pixels, pooling fix-ups) take the same table: a patch computes
// the pixels [y0, y1) x [x0, x1) of its segment, a patch no segment names computes nothing.  A thread whose pixels lie outside its
// patch's box returns before its first load; border tests stay against the patch.
struct RoiBox { int y0, y1, x0, x1; };
#ifdef __HIPCC__
#define TMAT_HD __host__ __device__ __forceinline__
#else
#define TMAT_HD inline
#endif
// The product form, for the kernels whose tables may name a patch range several times (depthwise and pooling of the unfused level; stem at
// the even pixels and pooling fix-up since the fused levels' rectangle launches have their shared-interior form): the
// segments of one patch are at most two row intervals times at most two column intervals (one segment: both intervals of an axis coincide).
struct RoiBox2 {
    int y0, y1, x0, x1;             // first row interval [y0, y1), first column interval [x0, x1)
    int y2, y3, x2, x3;             // second ones (copies of the first where the patch has one)
    // rows / columns of the box: both intervals of an axis, the second counted where the patch has one
    TMAT_HD int rows() const { return y1 - y0 + (y2 != y0 ? y3 - y2 : 0); }
    TMAT_HD int cols() const { return x1 - x0 + (x2 != x0 ? x3 - x2 : 0); }
#ifdef __HIPCC__
    __device__ __forceinline__ bool row(int y) const { return (y >= y0 && y < y1) || (y >= y2 && y < y3); }
    __device__ __forceinline__ bool col(int x) const { return (x >= x0 && x < x1) || (x >= x2 && x < x3); }
    // does [a, b) meet a row interval?
    __device__ __forceinline__ bool rows_meet(int a, int b) const { return (a < y1 && b > y0) || (a < y3 && b > y2); }
#endif
};
struct RoiNone {};
#ifdef __HIPCC__
// the box of patch n (n and the table are uniform: scalar compares); false: nothing to compute
__device__ __forceinline__ bool roi_box_of(const RoiSegs &r, int n, RoiBox &q)
{
    bool hit = false;
    q = RoiBox{0, 0, 0, 0};
    for (int k = 0; k < r.nseg; k++)
        if (n >= r.s[k].p0 && n < r.s[k].p0 + r.s[k].np) { q = RoiBox{r.s[k].y0, r.s[k].y0 + r.s[k].rh, r.s[k].x0, r.s[k].x0 + r.s[k].rw}; hit = true; }
    return hit;
}
// the same in the product form: two more scalar compares per axis
__device__ __forceinline__ bool roi_box_of(const RoiSegs &r, int n, RoiBox2 &q)
{
    bool hit = false;
    q = RoiBox2{0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < r.nseg; k++)
        if (n >= r.s[k].p0 && n < r.s[k].p0 + r.s[k].np) {
            const int y0 = r.s[k].y0, y1 = y0 + r.s[k].rh, x0 = r.s[k].x0, x1 = x0 + r.s[k].rw;
            if (!hit) q = RoiBox2{y0, y1, x0, x1, y0, y1, x0, x1};
            if (y0 != q.y0) { q.y2 = y0; q.y3 = y1; }
            if (x0 != q.x0) { q.x2 = x0; q.x3 = x1; }
            hit = true;
        }
    return hit;
}
__device__ __forceinline__ bool roi_box_of(const RoiNone &, int, RoiBox2 &) { return true; }
__device__ __forceinline__ bool roi_box_of(const RoiNone &, int, RoiBox &) { return true; }
#endif
// The COMPACT grids of the region form (stem at the even pixels, pooling fix-up): the workgroups of a patch enumerate the positions of the
// patch's own box, not of the frame.  Blocks per patch: enough for the largest box of the table -- positions(box) thread positions of C4
// threads each -- leaving out the boxes that are a whole frame (the all-constant patches, a few per pass: their workgroups take further
// steps of the grid) unless every box is one.  The segments that name one patch range stand together in the table.
template <class F>
inline int roi_compact_blocks(const RoiSegs &r, int frame_h, int frame_w, int C4, F positions)
{
    long long best = 0, whole = 0;
    for (int i = 0; i < r.nseg;) {
        RoiBox2 q{};
        int j = i;
        for (; j < r.nseg && r.s[j].p0 == r.s[i].p0; j++) {     // (the rule of roi_box_of)
            const int y0 = r.s[j].y0, y1 = y0 + r.s[j].rh, x0 = r.s[j].x0, x1 = x0 + r.s[j].rw;
            if (j == i) q = RoiBox2{y0, y1, x0, x1, y0, y1, x0, x1};
            if (y0 != q.y0) { q.y2 = y0; q.y3 = y1; }
            if (x0 != q.x0) { q.x2 = x0; q.x3 = x1; }
        }
        const long long n = positions(q);
        if (q.rows() >= frame_h && q.cols() >= frame_w) whole = n; else best = best > n ? best : n;
        i = j;
    }
    if (best == 0) best = whole;
    const long long blocks = (best * C4 + 255) / 256;
    return (int)(blocks < 1 ? 1 : blocks);
}
// returns false (and sets the error) on unsupported shapes; roi (nullable; stride 2 with the 1x1 form only: the rectangles are output
// pixels): region form
bool launch_conv(const ConvArgs &a, hipStream_t s, const RoiSegs *roi = nullptr);
// launch_conv's shape rule (pointers are only tested for null): cin % 64 == 0 for ksize 1 and 3, % 32 for the sub-pixel form, cout % 64 == 0, ...
bool conv_mfma_takes(const ConvArgs &a);
// The narrow layers' convolution (conv_narrow_kernels.hip), f32 contract only (prec 0): Cin and Cout multiples of 16, both >= 16, and
// everything else of launch_conv's contract -- ksize 3 stride 1; ksize 1 stride 1 or 2 (even sizes); ksize 2 without resid / out_relu;
// relu_in, nullable scale, resid with rs 0 or 1, relu_out, out_relu; Wo >= 2; M < 2^30; roi: the same table with the same meaning, any
// first column and width.  The same bits as launch_conv where both take a shape.  False ("launch_conv_narrow: unsupported shape", before
// any launch) otherwise.  The UNet driver launches it where conv_mfma_takes says no.
bool conv_narrow_takes(const ConvArgs &a);
bool launch_conv_narrow(const ConvArgs &a, hipStream_t s, const RoiSegs *roi = nullptr);
// Convolution with f16 activations in memory (conv_f16act_kernels.hip; the invasion-depth classifier's TMAT_RESNET_PRECISION_F16ACT):
// in / resid / out NHWC IEEE binary16 bits, W the f16 plane [ksize*ksize][Cout][Cin], scale (nullable) / shift f32.  ksize 1 (stride 1
// or 2) or 3 (stride 1), Cin and Cout multiples of 64.  Returns false (and sets the error) on unsupported shapes.
struct ConvF16Args {
    const uint16_t *in;
    int N, h, w, Cin;
    int ksize, stride;
    const uint16_t *W;
    int Cout;
    const float *scale;
    const float *shift;
    const uint16_t *resid;   // nullable, shaped like out
    int relu_out;
    uint16_t *out;           // (N, h/stride, w/stride, Cout)
};
bool launch_conv_f16act(const ConvF16Args &a, hipStream_t s);
// strips of the pooled separable convolution (floats): sepconv_ws_kernels.hip
size_t sepconv_pool_scratch_floats(int N, int H, int W, int Cout, bool quad = false);
// fused SeparableConv2D, wave-specialised (sepconv_ws_kernels.hip): depthwise taps dw9 [9][Cin], pointwise pwk [Cout][Cin] (k contiguous);
// the pooled form fuses MaxPooling2D(3, 2, "same") + the residual add behind it: out (N, H/2, W/2, Cout), scratch: sepconv_pool_scratch_floats
bool sepconv_ws_supported(int H, int W, int Cin, int Cout);
bool launch_sepconv_ws(const float *in, int N, int H, int W, int Cin, int relu_in, const float *dw9, const float *pwk, int Cout,
                       const float *scale, const float *shift, int relu_out, float *out, hipStream_t s, int prec = 0,
                       const int *tiles = nullptr, int n_tiles = 0, bool quad = false);
bool launch_sepconv_pool_ws(const float *in, int N, int H, int W, int Cin, int relu_in, const float *dw9, const float *pwk, int Cout,
                            const float *scale, const float *shift, int relu_out, float *scratch, const float *resid, float *out, hipStream_t s, int prec = 0,
                            const RoiSegs *roi_fix = nullptr,       // roi_fix: pooled pixels the fix-up pass finishes
                            const int *tiles = nullptr, int n_tiles = 0, bool quad = false);
// tiles (nullable, prec 0 only; here, above and in the stem form): region form of the convolution itself -- a device table of the n_tiles
// full-frame 16 x 16 tile ids (patch * tiles per patch + ty * tiles per row + tx) the launch visits (roi_plan.h:roi_sep_tile_table);
// the other tiles' outputs and strips stay unwritten
// quad (f32 path, with tiles): the table holds n_tiles PACKED tiles of four full-frame 8 x 8 quadrant ids each (patch * quadrants per
// patch + qy * quadrants per row + qx; roi_plan.h:roi_sep_quad_table, roi_sep_quad_pool_table) -- any four quadrants, of any patches; the
// others stay unwritten.  The pooled form then keeps its strips per quadrant (scratch: sepconv_pool_scratch_floats(.., true)) and its
// fix-up pass finishes the quadrant edges
// roi (nullable, here and below): the region form -- rows of a strip outside the box are neither loaded for nor computed
void launch_dwconv(const float *in, int N, int H, int W, int C, int relu_in, const float *Wd, float *out, hipStream_t s, const RoiSegs *roi = nullptr);
void launch_stem(const float *x, int N, int H, int W, const float *Ws, int Cout, const float *scale,
                 const float *shift, float *out, hipStream_t s);
// the stem at the even output pixels only: out (N, H/4, W/4, Cout); the input of block 0's stride-2 residual convolution when the stem
// itself is recomputed inside the first separable convolution (launch_sepconv_ws_stem)
void launch_stem_even(const float *x, int N, int H, int W, const float *Ws, int Cout, const float *scale,
                      const float *shift, float *out, hipStream_t s, const RoiSegs *roi = nullptr);
// SeparableConv2D over the stem's output WITHOUT the stem tensor in memory: x (N, 2H, 2W) single-channel patches; the depthwise
// producers recompute stem = relu(bn(conv3x3/s2(x))) (H x W x Cin) for their halo.  Same results as launch_stem + launch_sepconv_ws.
bool launch_sepconv_ws_stem(const float *x, int N, int H, int W, int Cin, const float *stem_w, const float *stem_scale, const float *stem_shift,
                            const float *dw9, const float *pwk, int Cout, const float *scale, const float *shift, int relu_out, float *out,
                            hipStream_t s, const int *tiles = nullptr, int n_tiles = 0, bool quad = false);
void launch_maxpool_add(const float *p2, int N, int H, int W, int C, const float *r, float *out, hipStream_t s, float *out_relu = nullptr,
                        const RoiSegs *roi = nullptr);
// roi (nullable): workgroups whose 8 x 16 stored pixels lie outside their patch's rectangle return at once
void launch_final(const float *S, int N, int h, int w, int C, const float *Wf, float bias, float *out, hipStream_t s, const RoiSegs *roi = nullptr);

// ---- constant-ring form of the down path (const_fill_kernels.hip; roi_plan.h:RoiDownPlan::fill) ----
// one strip of one class: the patches [p0, p0 + np), cnt per image in image order, take the pixels [y0, y0 + rh) x [x0, x0 + rw), all
// channels, from the all-constant patch src0 + (patch - p0) / cnt of the same tensor
struct FillItem { int p0, np, cnt, y0, x0, rh, rw; };
struct FillItems { int n; FillItem it[64]; };
// t (N, H, H, C), C % 4 == 0; false (and the error set) when an item leaves the tensor
bool launch_const_fill(float *t, int src0, int N, int H, int C, const FillItems &f, hipStream_t s);
// ---- shared-interior form (roi_plan.h:RoiDownPlan::share_fill) ----
// one rectangle of one class: the patches [p0, p0 + np) take the pixels [y0, y0 + rh) x [x0, x0 + rw), all channels, from their
// neighbour nbr[3 patch + dir] (dir 0 right, 1 below, 2 diagonal) at (y, x - H / 2), (y - H / 2, x), (y - H / 2, x - H / 2)
struct ShareItem { int p0, np, dir, y0, x0, rh, rw; };
// the launcher's host-side checks: false (and the error set) for an item that leaves its tensor, a source patch out of range, or a
// source rectangle that overlaps a destination rectangle of the patch it is read from
bool share_fill_check(int N, int H, int C, const int *nbr, const ShareItem *it, int n);
// t (N, H, H, C), C % 4 == 0; the neighbour table [N][3] and the n items on the host (checked) and on the device (read by the kernel)
bool launch_share_fill(float *t, int N, int H, int C, const int *nbr_host, const int *nbr_dev, const ShareItem *it_host, const ShareItem *it_dev, int n,
                       hipStream_t s);
// out (k, pp): patch i filled with padval[i]; pp % 4 == 0
void launch_const_patches(const float *padval, int k, int pp, float *out, hipStream_t s);

// ---- tiling / blending (blend_kernels.hip) -------------------------------------------------
// x: (n, hh, ww) f32; padval[n]; patches out: (n, 8, na_g, nb_g, ws, ws)
struct TileGeom {
    int hh, ww;     // image
    int ws, step, aug;
    int Hp, Wp;     // padded
    int na[2], nb[2];   // tile counts for even (k=0,2) / odd (k=1,3) rotations
    int tiles_per_img;  // sum over 8 orientations
    int tile_off[8];    // first tile index of orientation g within the image
    // Patch order of a pass of k images.  Null: image-major, patch = img tiles_per_img + tile.  Else the class-major order of the region
    // plan (roi_plan.h), a device table [tiles_per_img] of (class base, class count, rank in class, 0): patch = k base + img count + rank.
    const int4 *order;
};
TileGeom make_geom(int hh, int ww, int ws);
void launch_minmax_f32(const float *x, int n, size_t per, float *mn, float *mx, hipStream_t s);
void launch_norm_f32(float *x, size_t n, float mean, float sd, hipStream_t s);          // x = (x - mean) / sd in place
void launch_extract_tiles(const float *x, const float *padval, int n, const TileGeom &g, float *patches, hipStream_t s);
void launch_blend(const float *pred_patches, const double *win1d, int n, const TileGeom &g, double *out, hipStream_t s);

// ---- smooth tiling for any window size and subdivision count (smooth_kernels.hip) -----------
// One image.  Tile index: orientation-major, then a, then b (TileGeom's, image-major); a frame's tiles start at a step, b step for
// a in [0, na), b in [0, nb), and the strip behind the last tile belongs to no tile when the step does not divide the frame.
struct SmoothGeom {
    int hh, ww;
    int ws, sub, step, aug;
    int Hp, Wp;
    int na[2], nb[2];       // even / odd rotations
    int tile_off[8];
    int n_tiles;
};
// false (and the error set) for the geometries the stage refuses: ws < 4, sub < 2, sub > ws, an image side < 1, a frame side < ws,
// or more tiles than an int counts
bool smooth_geom(int hh, int ww, int ws, int sub, SmoothGeom &g);
// patches (count, ws, ws): the tiles [first, first + count) of x (hh, ww) padded with padval[0]
void launch_smooth_tiles(const float *x, const float *padval, const SmoothGeom &g, int first, int count, float *patches, hipStream_t s);
// pred (n_tiles, ws, ws) f32 (f64: pred_f64) -> out (hh, ww) f64
void launch_smooth_blend(const void *pred, bool pred_f64, const double *win1d, const SmoothGeom &g, double *out, hipStream_t s);
void launch_widen_f32(const float *in, double *out, size_t n, hipStream_t s);

// ---- ordered medial-axis thinning on the device (thin_kernels.hip) ------------------------------------
bool thin_dev_supported(int H, int W);
size_t thin_workspace_bytes(int n, int H, int W);
int thin_count_dev(const uint8_t *mask, int n, int H, int W, int *nfg, hipStream_t s);
struct ThinLayout {          // thin_dev's workspace
    uint64_t *keys;          // (n, H, W) order keys, ~0 on the background
    uint8_t *sd, *sd2, *dep; // (n, H, W) each: the two (value, done) snapshots, the predecessor bytes
    int *flags, *chunk, *tprog;
    uint8_t *tile_final, *tile_left;
    int nchunk;
    size_t tiles;
};
ThinLayout thin_layout(void *ws, int n, int H, int W);
int thin_dev(const uint8_t *mask, const double *dist, const uint32_t *tie, const int *nfg, int n, int H, int W, void *ws,
             const uint32_t *table_dev, uint8_t *skel, hipStream_t s, int *launches = nullptr);

// ---- DMT front end on the device (dmt_kernels.hip) -------------------------------------------------
inline size_t dmt_edge_count(int R, int C) { return (size_t)(R - 1) * C + (size_t)R * (C - 1) + (size_t)(R - 1) * (C - 1); }
size_t dmt_workspace_bytes(int n, int R, int C);
int dmt_sorted_edges_dev(const float *field, int n, int R, int C, void *ws, int32_t *ids, int *m, hipStream_t s);
// the two persistence sweeps on the device as levels of data-parallel steps, one workgroup per image (dmt_sweep_kernels.hip;
// TMAT_DMT_SWEEP_DEVICE=0 keeps them on host threads)
size_t dmt_sweep_workspace_bytes(int n, int R, int C);
int dmt_sweeps_dev(const float *field, const int32_t *ids, const int *m, int n, int R, int C, void *ws, uint8_t *kind, float *pers, hipStream_t s);

}  // namespace tmat
