// Tree overlay rasteriser (DESIGN.md "Tree overlay and barcode pictures"): declarations shared by overlay.cpp (host twin, C-ABI)
// and overlay_kernels.hip (device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace tmat {

// one drawn segment in canvas coordinates (float32, already mapped from background pixels) with its branch colour
struct OverlaySeg {
    float x1, y1, x2, y2;
    float r, g, b;          // 0..255, exact integers
    float pad;
};

constexpr int OVL_TW = 64, OVL_TH = 16;     // canvas tile of one workgroup

// Every formula of the picture specification, shared by the host twin and the kernels: float32, one operation per statement,
// no contraction (the build passes -ffp-contract=off).
__host__ __device__ inline int ovl_sample_index(int p, int src, int dst)
{
    float a = (float)p + 0.5f;
    float b = a * (float)src;
    float c = b / (float)dst;
    float u = c - 0.5f;
    float v = floorf(u + 0.5f);
    int k = (int)v;
    return k < 0 ? 0 : (k > src - 1 ? src - 1 : k);
}

// grey byte of a background value v for the image's minimum mn and maximum mx (a constant image gives 0)
__host__ __device__ inline float ovl_grey(float v, float mn, float mx)
{
    float range = mx - mn;
    if (!(range > 0.0f)) return 0.0f;
    float a = v - mn;
    float t = a / range;
    float s = t * 255.0f;
    return floorf(s + 0.5f);
}

// coverage of the pixel centre (cx, cy) by the capsule of segment s; rp = half-width + 0.5
__host__ __device__ inline float ovl_coverage(const OverlaySeg &s, float cx, float cy, float rp)
{
    float dx = s.x2 - s.x1;
    float dy = s.y2 - s.y1;
    float dxx = dx * dx;
    float dyy = dy * dy;
    float len2 = dxx + dyy;
    float px = cx - s.x1;
    float py = cy - s.y1;
    float t = 0.0f;
    if (len2 > 0.0f) {
        float pdx = px * dx;
        float pdy = py * dy;
        float dot = pdx + pdy;
        t = dot / len2;
        t = fminf(fmaxf(t, 0.0f), 1.0f);
    }
    float tx = t * dx;
    float ty = t * dy;
    float ex = px - tx;
    float ey = py - ty;
    float exx = ex * ex;
    float eyy = ey * ey;
    float d = sqrtf(exx + eyy);
    float a = rp - d;
    return fminf(fmaxf(a, 0.0f), 1.0f);
}

__host__ __device__ inline float ovl_blend(float C, float col, float a)
{
    float diff = col - C;
    float step = a * diff;
    return C + step;
}

// canvas of a (bh, bw) background at vis_width: vw, vh = round_half_even(vw bh / bw), rp = capsule half-width + 0.5; false when empty
struct Canvas { int vh, vw; float rp; };
bool canvas_of(int bh, int bw, int vis_width, Canvas &cv);
// background pixels -> canvas coordinates (float32) + branch colour, appended to out; segments with a non-finite coordinate are dropped
int prep_segments(const double *segs, const int32_t *seg_branch, int count, int bh, int bw, const Canvas &cv, std::vector<OverlaySeg> &out);

// background minima / maxima (mnmx: [n][2] floats) and the overlay of n images; bg_dtype 0: u16, 1: f32.  0 on success.
int overlay_minmax_dev(const void *bg, int bg_dtype, int n, int bh, int bw, float *mnmx, hipStream_t s);
int overlay_render_dev(const void *bg, int bg_dtype, const float *mnmx, int n, int bh, int bw, const OverlaySeg *segs, const int *seg_offsets,
                       int vh, int vw, float rp, uint8_t *rgb, hipStream_t s);

// What the "with tree" forms of the batch pipelines share (pipeline.cpp: 2-D images; stack_pipeline.cpp: Z stacks).
// tmat_morse_tree of one (threshold pair, image) item: the row, the bars into the caller's (cap_b, 2) block and the segments into vectors
// sized for the item (a forest has fewer edges than vertices)
int morse_tree_item(const int32_t *verts, int nv, const int32_t *edges, int ne, int fh, int fw, int smooth, int min_len, int max_len, int remove_isolated,
                    const uint8_t *pruning, double scaling_factor, int64_t *count, double *total_px, double *avg_px, std::vector<double> &segs,
                    std::vector<int32_t> &branch, double *bars, int cap_b, int *n_bars);
// device scratch of one pair's overlays of a pass of up to K images: segment table (seg_cap entries), (K, 2) extrema, K + 1 offsets, K canvases
struct OverlayWs { OverlaySeg *dseg; size_t seg_cap; float *dmm; int *doff; uint8_t *drgb; };
// One pair's overlays of the k images of a pass on stream s: item i's segments (segs[i], branch[i], background pixels) are mapped onto
// the canvas, uploaded and rasterised over bg (k, bh, bw) -- whose extrema overlay_minmax_dev has left in ws.dmm -- into ws.drgb; with
// rgb_host they are copied there.  Nothing is synchronised: ss and off are the host tables of the uploads and must live until the
// stream has drained.  TMAT_OK, TMAT_E_CAP (segment table too short) or TMAT_E_HIP, with the error set under `who`.
int overlay_pair_dev(const void *bg, int bg_dtype, int k, int bh, int bw, const Canvas &cv, const std::vector<double> *segs,
                     const std::vector<int32_t> *branch, const OverlayWs &ws, std::vector<OverlaySeg> &ss, std::vector<int> &off, uint8_t *rgb_host,
                     const char *who, hipStream_t s);

// Barcode picture (tmat_host_render_barcode / tmat_render_barcode): the host keeps the stable sort by birth, the edge rounding and the
// branch colours, and emits one rectangle per bar; host twin and barcode_kernel only fill them over a white S x S canvas.
// Columns [xa, xb), rows [ya, yb) counted from the BOTTOM row of the canvas; rgb = r | g << 8 | b << 16.  Entry k of a picture's table is
// row k of the sorted order: its rows lie inside [k pitch, (k + 1) pitch), pitch = S / n, and the rows of different bars are disjoint.
struct BarRect { int xa, xb, ya, yb; uint32_t rgb; };
int barcode_side(int vis_width);        // S = round_half_even(0.9 vis_width)
// appends the n rectangles of one picture to out -- or none when nothing is drawn (n == 0, a span that is zero or not finite)
void barcode_rects(const double *bars, int n, int S, std::vector<BarRect> &out);
void barcode_fill_host(const BarRect *rects, int n, int S, uint8_t *rgb);
// n_pics canvases (n_pics, S, S, 3) on the device from the concatenated tables; picture p owns [rect_off[p], rect_off[p + 1]).  0 on success.
int barcode_render_dev(const BarRect *rects, const int *rect_off, int n_pics, int S, uint8_t *rgb, hipStream_t s);

}  // namespace tmat
