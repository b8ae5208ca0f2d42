// Region planner of the UNet up path: see roi_plan.h.  Host arithmetic only.
#include "roi_plan.h"
#include "tmat_internal.h"
#include "../../include/tmat.h"

#include <algorithm>

namespace tmat {

namespace {

struct Iv { int lo, hi; };      // [lo, hi)

Iv clip(Iv v, int R) { return Iv{std::max(v.lo, 0), std::min(v.hi, R)}; }
Iv dilate(Iv v, int d, int R) { return clip(Iv{v.lo - d, v.hi + d}, R); }
Iv hull(Iv a, Iv b) { return Iv{std::min(a.lo, b.lo), std::max(a.hi, b.hi)}; }
// the half-resolution pixels that the pixels of v sit on (x >> 1)
Iv halve(Iv v) { return Iv{v.lo >> 1, (v.hi + 1) >> 1}; }
// Columns, rounded outwards to what conv_mfma_kernel's row-uniform prologue and epilogue want: first column a multiple of 4 (the
// low-resolution residual pairs columns), width a multiple of 8 (8 consecutive pixels of a DMA pass lie in one row) -- or the whole row.
// Below 64 pixels a side the width is a multiple of 4 only: 8 columns are a fifth of a 40-pixel row, while the per-lane prologue such a
// width falls back to is ~35 vector instructions per DMA pass beside the >= 2048-deep contractions of those levels (0.75 % of a tile by
// the 3 % measured at K = 576); the epilogue's 4-pixel row groups stay row-uniform.
Iv align_cols(Iv v, int R)
{
    int lo = v.lo & ~3, hi = std::min(R, (v.hi + 3) & ~3);
    if (R >= 64 && ((hi - lo) & 7) != 0) {
        if (lo >= 4) lo -= 4;
        else if (hi + 4 <= R) hi += 4;
        else { lo = 0; hi = R; }
    }
    return Iv{lo, hi};
}
Iv round_cols(Iv v, int R, bool exact) { return exact ? v : align_cols(v, R); }
// align_cols kept inside `outer`, a rectangle of that form around v: a width that is 4 short of a multiple of 8 grows to the left where
// outer has the room, else to the right (outer is 4 wider than the 4-aligned v at least, on one side or the other)
Iv align_cols_in(Iv v, int R, Iv outer)
{
    Iv q = align_cols(v, R);
    if (q.lo < outer.lo) q = Iv{q.lo + 4, q.hi + 4};
    return q;
}
Iv align_to(Iv v, int al, int R) { return Iv{v.lo / al * al, std::min(R, (v.hi + al - 1) / al * al)}; }

// one class: rows[l] / cols[l] for every layer, from the interval of final outputs the blend reads on each axis
// exact: no rounding -- the pixels the blend DEPENDS on (the down plan starts from those: roi_plan_down)
// parity (with exact): a sub-pixel layer's read of the previous block's output follows the parity of its outputs -- output 2 i + p sees
// the stored pixels i + p - 1 and i + p, so the outputs [lo, hi) see [(lo - 1) >> 1, (hi >> 1) + 1) -- where the plain walk takes one pixel
// around the stored pixels that make those outputs (one more on a side whose first output is odd / whose last is even).  The exact
// rectangles of the up plan use it; the tight rectangles and the down plan keep the plain walk they were built on.
void walk_back(Iv orow, Iv ocol, int ws, int n_up, Iv *rows, Iv *cols, bool exact = false, bool parity = false)
{

    const int L = 3 * n_up + 1;
    int R = ws / 2;                                          // stored resolution of the final convolution
    // final_kernel: one thread = the 2 x 2 outputs above a stored pixel, one workgroup = 8 x 16 stored pixels, skipped or run as a whole
    rows[L - 1] = exact ? halve(orow) : align_to(halve(orow), 8, R);
    cols[L - 1] = exact ? halve(ocol) : align_to(halve(ocol), 16, R);
    Iv need_r = dilate(rows[L - 1], 1, R), need_c = dilate(cols[L - 1], 1, R);      // of the last block's output
    for (int j = n_up - 1; j >= 0; j--) {
        const int Hl = R, Hs = j ? R / 2 : R;
        // second 3x3 (writes the block output and its activated copy): reads t1 one pixel around, the residual at (y >> up, x >> up)
        const Iv c2r = need_r, c2c = round_cols(need_c, Hl, exact);
        rows[3 * j + 2] = c2r; cols[3 * j + 2] = c2c;
        const Iv t1r = dilate(c2r, 1, Hl), t1c = dilate(c2c, 1, Hl);
        const Iv rsr = j ? halve(c2r) : c2r, rsc = round_cols(j ? halve(c2c) : c2c, Hs, exact);
        rows[3 * j + 1] = rsr; cols[3 * j + 1] = rsc;
        // first convolution.  Sub-pixel form (j > 0): stored pixel i makes the outputs 2 i and 2 i + 1 from the stored pixels i - 1 .. i + 1
        const Iv c1r = j ? halve(t1r) : t1r, c1c = round_cols(j ? halve(t1c) : t1c, Hs, exact);
        rows[3 * j] = c1r; cols[3 * j] = c1c;
        // what the block reads of the previous block's output: the residual 1x1 its plain form, the first convolution its activated copy
        const bool sub = exact && parity && j;
        need_r = hull(rsr, sub ? clip(Iv{(t1r.lo - 1) >> 1, (t1r.hi >> 1) + 1}, Hs) : dilate(c1r, 1, Hs));
        need_c = hull(rsc, sub ? clip(Iv{(t1c.lo - 1) >> 1, (t1c.hi >> 1) + 1}, Hs) : dilate(c1c, 1, Hs));
        R = Hs;
    }
}

// one axis of one class through the down path: need[l] / rect[l] for every layer of RoiDownPlan, from the interval `out` of the
// bottleneck tensor that up block 0 reads
void walk_down_axis(Iv out, bool cols, int ws, int n_down, unsigned fused_mask, Iv *need, Iv *rect)
{
    for (int b = n_down - 1; b >= 0; b--) {
        const int H = (ws / 2) >> b, Ho = H / 2;
        Iv *nd = need + 6 * b, *rc = rect + 6 * b;
        nd[5] = rc[5] = out;                                     // max-pool + add: one thread per pixel
        nd[4] = out;                                             // the residual 1x1 makes the pixels the add takes
        rc[4] = cols ? align_cols(out, Ho) : out;
        // MaxPooling2D(3, 2, "same") on an even side pads behind only (oracle/unet_exact.c:orc_maxpool_add): output i reads 2 i .. 2 i + 2
        nd[3] = nd[2] = clip(Iv{2 * out.lo, 2 * out.hi + 1}, H);
        nd[1] = nd[0] = dilate(nd[2], 1, H);
        for (int k = 0; k < 4; k++)
            rc[k] = ((fused_mask >> b) & 1u) ? align_to(nd[k], 16, H) : cols ? align_cols(nd[k], H) : nd[k];
        // the block's input: one pixel around the first depthwise layer's needed outputs, and the even pixels under the stride-2 residual
        out = hull(dilate(nd[0], 1, H), Iv{2 * out.lo, 2 * out.hi - 1});
    }
    const int L = 6 * n_down;
    need[L + 3] = rect[L + 3] = Iv{0, 0};                        // (the blend's own rectangle: filled by the caller)
    need[L] = need[4]; rect[L] = rect[4];                        // the stem at its even pixels: exactly what block 0's residual 1x1 enumerates
    need[L + 1] = out;
    rect[L + 1] = (fused_mask & 1u) ? dilate(rect[0], 1, ws / 2) : Iv{0, ws / 2};       // recomputed under the first depthwise tiles' halos, or the whole stem tensor
    // Conv2D(3, strides 2, "same") on an even side: stem pixel i reads input 2 i .. 2 i + 2
    need[L + 2] = clip(Iv{2 * out.lo, 2 * out.hi + 1}, ws);
    rect[L + 2] = Iv{0, ws};                                     // the tile gather writes whole patches
}

// The taps of the down path for the constant-ring form: output pixel i of a layer reads its producer at s i + a .. s i + b (one axis).
struct Tap { int s, a, b; };
constexpr Tap TAP_DW{1, -1, 1};         // depthwise 3 x 3, "same"
constexpr Tap TAP_PW{1, 0, 0};          // pointwise, and the residual under the add
constexpr Tap TAP_EVEN{2, 0, 0};        // the stride-2 residual 1x1, the stem at its even pixels
constexpr Tap TAP_S2{2, 0, 2};          // MaxPooling2D(3, 2, "same") and the stem's Conv2D(3, strides 2, "same") on an even side

bool empty(Iv v) { return v.hi <= v.lo; }
Iv hull_e(Iv a, Iv b) { return empty(a) ? b : empty(b) ? a : hull(a, b); }
Iv meet(Iv a, Iv b) { const Iv v{std::max(a.lo, b.lo), std::min(a.hi, b.hi)}; return empty(v) ? Iv{0, 0} : v; }
int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// the outputs in [0, R) of which some tap lies in v
Iv tap_fwd(Iv v, Tap t, int R)
{
    if (empty(v)) return Iv{0, 0};
    const Iv o = clip(Iv{-floor_div(-(v.lo - t.b), t.s), floor_div(v.hi - 1 - t.a, t.s) + 1}, R);
    return empty(o) ? Iv{0, 0} : o;
}
// the hull of the taps of the outputs v, clipped to the producer's side R
Iv tap_back(Iv v, Tap t, int R)
{
    if (empty(v)) return Iv{0, 0};
    const Iv o = clip(Iv{t.s * v.lo + t.a, t.s * (v.hi - 1) + t.b + 1}, R);
    return empty(o) ? Iv{0, 0} : o;
}

// One axis of one class in the constant-ring form.  rd: the part of the input window that is image data.  need / rect: walk_down_axis.
// Out: nonconst, live, rect_live and reads (the hull of the taps of the consumers' live: live ∪ fill of a stored tensor) per layer.
void walk_const_axis(Iv rd, bool cols, int ws, int n_down, unsigned fused_mask, const Iv *need, const Iv *rect, Iv *nc, Iv *live, Iv *rl, Iv *reads)
{
    const int L = 6 * n_down;
    // forwards: what the image data reaches
    nc[L + 3] = nc[L + 2] = rd;
    nc[L + 1] = tap_fwd(rd, TAP_S2, ws / 2);
    nc[L] = tap_fwd(nc[L + 1], TAP_EVEN, ws / 4);
    Iv in = nc[L + 1];
    for (int b = 0; b < n_down; b++) {
        const int H = (ws / 2) >> b, Ho = H / 2;
        Iv *q = nc + 6 * b;
        q[0] = tap_fwd(in, TAP_DW, H);
        q[1] = tap_fwd(q[0], TAP_PW, H);
        q[2] = tap_fwd(q[1], TAP_DW, H);
        q[3] = tap_fwd(q[2], TAP_PW, H);
        q[4] = tap_fwd(in, TAP_EVEN, Ho);
        q[5] = hull_e(tap_fwd(q[3], TAP_S2, Ho), tap_fwd(q[4], TAP_PW, Ho));
        in = q[5];
    }
    // backwards: a stored tensor computes need ∩ nonconst, a tensor that is never stored whatever its consumer's live reads
    for (int b = n_down - 1; b >= 0; b--) {
        const int H = (ws / 2) >> b, Ho = H / 2;
        const bool fused = (fused_mask >> b) & 1u;
        const Iv *nd = need + 6 * b, *q = nc + 6 * b;
        Iv *lv = live + 6 * b, *rd_ = reads + 6 * b;
        rd_[5] = b + 1 == n_down ? nd[5] : hull_e(tap_back(lv[6], TAP_DW, Ho), tap_back(lv[6 + 4], TAP_EVEN, Ho));
        lv[5] = meet(nd[5], q[5]);
        rd_[4] = tap_back(lv[5], TAP_PW, Ho);
        lv[4] = meet(nd[4], q[4]);
        rd_[3] = tap_back(lv[5], TAP_S2, H);
        lv[3] = fused ? rd_[3] : meet(nd[3], q[3]);
        rd_[2] = tap_back(lv[3], TAP_PW, H);
        lv[2] = fused ? rd_[2] : meet(nd[2], q[2]);
        rd_[1] = tap_back(lv[2], TAP_DW, H);
        lv[1] = meet(nd[1], q[1]);
        rd_[0] = tap_back(lv[1], TAP_PW, H);
        lv[0] = fused ? rd_[0] : meet(nd[0], q[0]);
    }
    reads[L] = tap_back(live[4], TAP_PW, ws / 4);
    live[L] = meet(need[L], nc[L]);
    reads[L + 1] = hull_e(tap_back(live[0], TAP_DW, ws / 2), tap_back(live[L], TAP_EVEN, ws / 2));
    live[L + 1] = (fused_mask & 1u) ? reads[L + 1] : need[L + 1];       // inside the STEM layer, or written whole by the stem's own kernel
    reads[L + 2] = tap_back(live[L + 1], TAP_S2, ws);
    live[L + 2] = need[L + 2];
    reads[L + 3] = live[L + 3] = need[L + 3];
    // live rounded by rect's rule (walk_down_axis), kept inside rect
    for (int b = 0; b < n_down; b++) {
        const int H = (ws / 2) >> b, Ho = H / 2;
        const bool fused = (fused_mask >> b) & 1u;
        for (int k = 0; k < 6; k++) {
            const int l = 6 * b + k;
            Iv v = live[l];
            if (!empty(v)) {
                if (k < 4 && fused) v = align_to(v, 16, H);
                else if (k < 5 && cols) v = align_cols_in(v, k < 4 ? H : Ho, rect[l]);
            }
            if (!empty(v) && (v.lo < rect[l].lo || v.hi > rect[l].hi)) v = rect[l];
            rl[l] = v;
        }
    }
    rl[L] = rl[4];
    rl[L + 1] = (fused_mask & 1u) ? (empty(rl[0]) ? Iv{0, 0} : dilate(rl[0], 1, ws / 2)) : rect[L + 1];
    rl[L + 2] = rect[L + 2];
    rl[L + 3] = rect[L + 3];
}

RoiRect rect_of(Iv r, Iv c) { return (empty(r) || empty(c)) ? RoiRect{0, 0, 0, 0} : RoiRect{r.lo, c.lo, r.hi - r.lo, c.hi - c.lo}; }

// q \ nc as strips: above, below, left, right of nc (empty strips have rh = rw = 0)
void fill_strips(RoiRect q, RoiRect nc, RoiRect *out)
{
    for (int i = 0; i < 4; i++) out[i] = RoiRect{0, 0, 0, 0};
    if (q.rh <= 0 || q.rw <= 0) return;
    const int y0 = std::max(q.y0, nc.y0), y1 = std::min(q.y0 + q.rh, nc.y0 + nc.rh);
    const int x0 = std::max(q.x0, nc.x0), x1 = std::min(q.x0 + q.rw, nc.x0 + nc.rw);
    if (nc.rh <= 0 || nc.rw <= 0 || y1 <= y0 || x1 <= x0) { out[0] = q; return; }
    if (y0 > q.y0) out[0] = RoiRect{q.y0, q.x0, y0 - q.y0, q.rw};
    if (y1 < q.y0 + q.rh) out[1] = RoiRect{y1, q.x0, q.y0 + q.rh - y1, q.rw};
    if (x0 > q.x0) out[2] = RoiRect{y0, q.x0, y1 - y0, x0 - q.x0};
    if (x1 < q.x0 + q.rw) out[3] = RoiRect{y0, x1, y1 - y0, q.x0 + q.rw - x1};
}

}  // namespace

bool roi_plan_down(RoiPlan &p, int n_down, const int *chan, unsigned fused_mask)
{
    p.down = RoiDownPlan();
    if (p.n_classes <= 0 || n_down < 1 || n_down > ROI_MAX_DOWN || n_down + 1 != p.n_up || !chan) return false;      // (ws is a multiple of 4 << n_up: roi_make_plan)
    for (int b = 0; b < n_down; b++)
        if (((fused_mask >> b) & 1u) && (((p.ws / 2) >> b) % 16) != 0) return false;
    RoiDownPlan &d = p.down;
    const int L = 6 * n_down, ws = p.ws;
    double mpp[ROI_MAX_DOWN_LAYERS] = {}, bpp[ROI_MAX_DOWN_LAYERS] = {};       // multiply-accumulates / bytes per enumerated pixel
    for (int b = 0; b < n_down; b++) {
        const int H = (ws / 2) >> b, cin = chan[b], cout = chan[b + 1];
        const bool fused = (fused_mask >> b) & 1u;
        for (int k = 0; k < 4; k++) d.res[6 * b + k] = H;
        d.res[6 * b + 4] = d.res[6 * b + 5] = H / 2;
        mpp[6 * b + 1] = (double)cin * cout; mpp[6 * b + 3] = (double)cout * cout; mpp[6 * b + 4] = (double)cin * cout;
        if (!fused) {           // the streaming kernels of an unfused level: depthwise reads and writes a pixel, the pooling reads 4 and the residual, writes 1
            bpp[6 * b] = 8.0 * cin; bpp[6 * b + 2] = 8.0 * cout; bpp[6 * b + 5] = 24.0 * cout;
        }
    }
    d.res[L] = ws / 4; d.res[L + 1] = ws / 2; d.res[L + 2] = ws;
    if (fused_mask & 1u) bpp[L] = 4.0 * chan[0];
    bpp[L + 2] = 4.0;
    d.res[L + 3] = ws;
    d.n_down = n_down; d.n_layers = L + 4; d.fused_mask = fused_mask;
    for (int b = 0; b < n_down; b++)
        for (int k = 0; k < 6; k++) d.stored[6 * b + k] = !((fused_mask >> b) & 1u) || k == 1 || k >= 4;
    d.stored[L] = true;         // (the stem and the input window are written whole)
    for (int l = 0; l < d.n_layers; l++) {
        d.mac_full[l] = mpp[l] * d.res[l] * d.res[l] * p.tiles_per_img;
        d.bytes_full[l] = bpp[l] * d.res[l] * d.res[l] * p.tiles_per_img;
    }
    const int R0 = ws >> p.n_up;
    for (int k = 0; k < p.n_classes; k++) {
        const RoiRect &rd = p.read[k];
        if (rd.rh <= 0 || rd.rw <= 0) continue;         // a class the blend reads nothing of: empty rectangles throughout
        // What the blend's rectangle DEPENDS on of the bottleneck tensor: the up path walked once more without its rounding (its kernels
        // compute the rounded rectangles of p.rect; their extra pixels may see operands the down path leaves unwritten, and feed nothing
        // the blend reads).  Up block 0 reads the plain tensor under its residual 1x1, the activated copy one pixel around its first 3x3.
        Iv ur[ROI_MAX_LAYERS], uc[ROI_MAX_LAYERS];
        walk_back(Iv{rd.y0, rd.y0 + rd.rh}, Iv{rd.x0, rd.x0 + rd.rw}, ws, p.n_up, ur, uc, true);
        const Iv orow = hull(ur[1], dilate(ur[0], 1, R0)), ocol = hull(uc[1], dilate(uc[0], 1, R0));
        Iv nr[ROI_MAX_DOWN_LAYERS], nc[ROI_MAX_DOWN_LAYERS], rr[ROI_MAX_DOWN_LAYERS], rc[ROI_MAX_DOWN_LAYERS];
        walk_down_axis(orow, false, ws, n_down, fused_mask, nr, rr);
        walk_down_axis(ocol, true, ws, n_down, fused_mask, nc, rc);
        nr[L + 3] = rr[L + 3] = Iv{rd.y0, rd.y0 + rd.rh}; nc[L + 3] = rc[L + 3] = Iv{rd.x0, rd.x0 + rd.rw};
        for (int l = 0; l < d.n_layers; l++) {
            d.need[l][k] = RoiRect{nr[l].lo, nc[l].lo, nr[l].hi - nr[l].lo, nc[l].hi - nc[l].lo};
            const RoiRect q{rr[l].lo, rc[l].lo, rr[l].hi - rr[l].lo, rc[l].hi - rc[l].lo};
            d.rect[l][k] = q;
            d.mac_planned[l] += mpp[l] * q.rh * q.rw * p.class_count[k];
            d.bytes_planned[l] += bpp[l] * q.rh * q.rw * p.class_count[k];
        }
        // the constant-ring form of the same class
        Iv cr[ROI_MAX_DOWN_LAYERS], cc[ROI_MAX_DOWN_LAYERS], lr[ROI_MAX_DOWN_LAYERS], lc[ROI_MAX_DOWN_LAYERS];
        Iv vr[ROI_MAX_DOWN_LAYERS], vc[ROI_MAX_DOWN_LAYERS], qr[ROI_MAX_DOWN_LAYERS], qc[ROI_MAX_DOWN_LAYERS];
        walk_const_axis(Iv{rd.y0, rd.y0 + rd.rh}, false, ws, n_down, fused_mask, nr, rr, cr, lr, vr, qr);
        walk_const_axis(Iv{rd.x0, rd.x0 + rd.rw}, true, ws, n_down, fused_mask, nc, rc, cc, lc, vc, qc);
        for (int l = 0; l < d.n_layers; l++) {
            d.nonconst[l][k] = rect_of(cr[l], cc[l]);
            d.live[l][k] = rect_of(lr[l], lc[l]);
            const RoiRect q = rect_of(vr[l], vc[l]);
            d.rect_live[l][k] = q;
            d.mac_live[l] += mpp[l] * q.rh * q.rw * p.class_count[k];
            d.bytes_live[l] += bpp[l] * q.rh * q.rw * p.class_count[k];
            if (d.stored[l]) fill_strips(rect_of(qr[l], qc[l]), d.nonconst[l][k], d.fill[l][k]);
        }
        for (int b = 0; b < n_down; b++)
            if ((fused_mask >> b) & 1u)
                for (int l = 6 * b + 1; l <= 6 * b + 3; l += 2)
                    if (d.rect[l][k].rh < d.res[l] || d.rect[l][k].rw < d.res[l]) d.free_tile[b] = true;
    }
    roi_plan_share(p);
    return true;
}

// ---- the shared-interior form (roi_plan.h:RoiDownPlan::share) ----
namespace {

typedef std::vector<unsigned char> Mask;

// the outputs in [0, R) of which EVERY tap lies in v (v inside the producer's side: a tap outside the tensor is outside v)
Iv tap_fwd_all(Iv v, Tap t, int R)
{
    if (empty(v)) return Iv{0, 0};
    const Iv o = clip(Iv{-floor_div(-(v.lo - t.a), t.s), floor_div(v.hi - 1 - t.b, t.s) + 1}, R);
    return empty(o) ? Iv{0, 0} : o;
}
Mask mask_of(Iv v, int R)
{
    Mask m(R, 0);
    for (int i = std::max(v.lo, 0); i < std::min(v.hi, R); i++) m[i] = 1;
    return m;
}
// the taps of the outputs in m, inside the producer's side R
Mask taps_of(const Mask &m, Tap t, int R)
{
    Mask o(R, 0);
    for (int i = 0; i < (int)m.size(); i++)
        if (m[i])
            for (int j = std::max(t.s * i + t.a, 0); j <= std::min(t.s * i + t.b, R - 1); j++) o[j] = 1;
    return o;
}
std::vector<Iv> runs_of(const Mask &m)
{
    std::vector<Iv> r;
    for (int i = 0; i < (int)m.size(); i++)
        if (m[i]) {
            if (!r.empty() && r.back().hi == i) r.back().hi = i + 1;
            else r.push_back(Iv{i, i + 1});
        }
    return r;
}
Iv longest_run(const Mask &m)
{
    Iv best{0, 0};
    for (const Iv &v : runs_of(m)) if (v.hi - v.lo > best.hi - best.lo) best = v;
    return best;
}
bool any(const Mask &m) { for (unsigned char c : m) if (c) return true; return false; }
unsigned long long tiles_touching(const Mask &m)
{
    unsigned long long t = 0;
    for (int i = 0; i < (int)m.size(); i++) if (m[i]) t |= 1ull << (i / 16);
    return t;
}

// one axis key: the interval of `read` on the axis, the patches that follow a patch of the key, and the key's sets per layer
struct AxisKey {
    Iv rd{0, 0};
    std::vector<int> next;                  // keys of the successors (no duplicates)
    bool last = false;                      // some patch of the key has no successor on the axis
    Iv live[ROI_MAX_DOWN_LAYERS] = {};
    Mask low[ROI_MAX_DOWN_LAYERS];          // stored tensors of the shared levels: what the patch computes of its lower half whatever it shares itself
    Iv share[ROI_MAX_DOWN_LAYERS] = {};
    Mask comp[ROI_MAX_DOWN_LAYERS], sfill[ROI_MAX_DOWN_LAYERS];
    unsigned long long tiles[ROI_MAX_DOWN_LAYERS] = {};     // ~0 where the key shares nothing at the level
    // the rectangle launches' form (RoiDownPlan::rcomp), layers 6 b + 0 .. 6 b + 5 of the last level
    Mask rlow, rc[6];
    Iv rshare{0, 0};
};

void inner_axis(int ws, int n_down, Iv *in)
{
    const int L = 6 * n_down;
    in[L + 3] = in[L + 2] = Iv{0, ws};
    in[L + 1] = tap_fwd_all(in[L + 2], TAP_S2, ws / 2);
    in[L] = tap_fwd_all(in[L + 1], TAP_EVEN, ws / 4);
    Iv prev = in[L + 1];
    for (int b = 0; b < n_down; b++) {
        const int H = (ws / 2) >> b, Ho = H / 2;
        Iv *q = in + 6 * b;
        q[0] = tap_fwd_all(prev, TAP_DW, H);
        q[1] = tap_fwd_all(q[0], TAP_PW, H);
        q[2] = tap_fwd_all(q[1], TAP_DW, H);
        q[3] = tap_fwd_all(q[2], TAP_PW, H);
        q[4] = tap_fwd_all(prev, TAP_EVEN, Ho);
        q[5] = meet(tap_fwd_all(q[3], TAP_S2, Ho), tap_fwd_all(q[4], TAP_PW, Ho));
        prev = q[5];
    }
}

bool in_iv(Iv v, int i) { return i >= v.lo && i < v.hi; }

// the level whose rectangle launches take the shared-interior form: the last one, unfused and in ROI_SHARE_RECT_LEVELS; -1: none
int share_rect_level(const RoiDownPlan &d)
{
    const int b = d.n_down - 1;
    return (b >= 0 && !((d.fused_mask >> b) & 1u) && ((ROI_SHARE_RECT_LEVELS >> b) & 1u)) ? b : -1;
}

// per key: rshare and the exact comp of the level's six layers (live where the key shares nothing)
void share_rect_keys(const RoiPlan &p, std::vector<AxisKey> &keys, const Iv *inner)
{
    const RoiDownPlan &d = p.down;
    const int b = d.n_down - 1, l0 = 6 * b, H = (p.ws / 2) >> b, Ho = H / 2;
    for (AxisKey &key : keys) key.rlow = mask_of(meet(key.live[l0 + 5], Iv{0, Ho / 2}), Ho);
    for (AxisKey &key : keys) {
        for (int kk = 0; kk < 6; kk++) key.rc[kk] = mask_of(key.live[l0 + kk], d.res[l0 + kk]);
        key.rshare = Iv{0, 0};
        if (share_rect_level(d) < 0 || key.last || key.next.empty() || empty(key.rd)) continue;
        Mask m(Ho, 0);
        for (int v = Ho / 2; v < Ho; v++) {
            bool ok = in_iv(key.live[l0 + 5], v) && in_iv(inner[l0 + 5], v) && in_iv(inner[l0 + 5], v - Ho / 2);
            for (size_t i = 0; ok && i < key.next.size(); i++) ok = keys[key.next[i]].rlow[v - Ho / 2];
            m[v] = ok;
        }
        const Iv sh = longest_run(m);
        if (empty(sh)) continue;
        Mask c[6];
        c[5] = key.rc[5];
        for (int v = sh.lo; v < sh.hi; v++) c[5][v] = 0;
        auto within = [](Mask a, const Mask &lv) { for (size_t i = 0; i < a.size(); i++) a[i] = a[i] && lv[i]; return a; };
        c[4] = within(c[5], key.rc[4]);                                 // the residual under the add (outside its live it is constant: fill)
        c[3] = within(taps_of(c[5], TAP_S2, H), key.rc[3]);             // the halo of the pooling joins comp
        c[2] = within(c[3], key.rc[2]);
        c[1] = within(taps_of(c[2], TAP_DW, H), key.rc[1]);             // the halo of the second depthwise layer joins comp
        c[0] = within(c[1], key.rc[0]);
        bool two = true;
        for (int kk = 0; kk < 6; kk++) two = two && runs_of(c[kk]).size() <= 2;
        if (!two) continue;
        key.rshare = sh;
        for (int kk = 0; kk < 6; kk++) key.rc[kk] = c[kk];
    }
}

// ---- what the three sharing forms build per class the same way ----
typedef RoiDownPlan::RectForm RectForm;

bool live_class(const RoiPlan &p, int k) { return p.class_count[k] > 0 && p.read[k].rh > 0 && p.read[k].rw > 0; }
unsigned char *mask_at(Mask &m, int ws, int l, int k, int axis) { return m.data() + (((size_t)l * ROI_MAX_CLASSES + k) * 2 + axis) * ws; }

// The copies of class k's tensor l out of its neighbours, the product of its axes: from the right neighbour the rows it computes itself
// by its shared columns, from the lower one its shared rows by its own columns, from the diagonal one shared by shared
void put_fills(std::vector<RoiDownPlan::ShareFill> &out, int l, int k, const std::vector<Iv> &own_rows, const std::vector<Iv> &got_rows,
               const std::vector<Iv> &own_cols, const std::vector<Iv> &got_cols)
{
    auto put = [&](int dir, const std::vector<Iv> &rows, const std::vector<Iv> &cols) {
        for (const Iv &r : rows)
            for (const Iv &c : cols) out.push_back(RoiDownPlan::ShareFill{l, k, dir, r.lo, c.lo, r.hi - r.lo, c.hi - c.lo});
    };
    put(0, own_rows, got_cols); put(1, got_rows, own_cols); put(2, got_rows, got_cols);
}

// The rectangles a class launches for an exact set, the product of at most two runs per axis: rows exact; round4: the columns rounded
// outwards to multiples of 4 inside rl (the class's rect_live), two runs that meet after rounding being one.  True: they are not rl itself.
bool launched_rects(const std::vector<Iv> &rows, std::vector<Iv> cols, bool round4, const RoiRect &rl, RoiRect *out, int &n)
{
    for (Iv &c : cols)
        if (round4) c = meet(Iv{c.lo & ~3, (c.hi + 3) & ~3}, Iv{rl.x0, rl.x0 + rl.rw});
    if (cols.size() == 2 && cols[0].hi >= cols[1].lo) { cols[0].hi = cols[1].hi; cols.pop_back(); }
    n = 0;
    for (const Iv &r : rows)
        for (const Iv &c : cols) out[n++] = RoiRect{r.lo, c.lo, r.hi - r.lo, c.hi - c.lo};
    return n != 1 || out[0].y0 != rl.y0 || out[0].x0 != rl.x0 || out[0].rh != rl.rh || out[0].rw != rl.rw;
}

// layer l of a form, once its rectangles stand: the totals, and the form's longest segment table
void tally(const RoiPlan &p, RectForm &f, int l)
{
    const RoiDownPlan &d = p.down;
    const double area = (double)d.res[l] * d.res[l] * p.tiles_per_img;
    const double mpp = area > 0 ? d.mac_full[l] / area : 0, bpp = area > 0 ? d.bytes_full[l] / area : 0;
    f.mac[l] = f.bytes[l] = f.px[l] = 0;
    int nseg = 0;
    for (int k = 0; k < p.n_classes; k++) {
        for (int i = 0; i < f.n[l][k]; i++) {
            const double px = (double)f.rects[l][k][i].rh * f.rects[l][k][i].rw * p.class_count[k];
            f.mac[l] += mpp * px; f.bytes[l] += bpp * px; f.px[l] += px;
        }
        if (p.class_count[k] > 0) nseg += f.n[l][k];
    }
    f.segs = std::max(f.segs, nseg);
}

// per class: the rectangles as launched, the copies of the bottleneck tensor, the totals (RoiDownPlan::rcomp)
void share_rect_classes(RoiPlan &p, const std::vector<AxisKey> &keys, const int *krow, const int *kcol)
{
    RoiDownPlan &d = p.down;
    RectForm &f = d.rcomp;
    const int NL = d.n_layers, ws = p.ws, bl = d.n_down - 1;
    f = RectForm();
    f.mask.assign((size_t)NL * ROI_MAX_CLASSES * 2 * ws, 0);
    // A class takes the form in all six layers of the level or in none (a layer that fell back to rect_live on its own would compute live
    // over producers whose comp was already cut): only where every layer's comp lies inside its rect_live
    bool takes[ROI_MAX_CLASSES] = {};
    for (int k = 0; k < p.n_classes; k++) {
        const AxisKey &kr = keys[krow[k]], &kc = keys[kcol[k]];
        takes[k] = bl >= 0 && live_class(p, k) && (!empty(kr.rshare) || !empty(kc.rshare));
        for (int kk = 0; takes[k] && kk < 6; kk++) {
            const RoiRect rl = d.rect_live[6 * bl + kk][k];
            for (const Iv &r : runs_of(kr.rc[kk])) takes[k] = takes[k] && r.lo >= rl.y0 && r.hi <= rl.y0 + rl.rh;
            for (const Iv &c : runs_of(kc.rc[kk])) takes[k] = takes[k] && c.lo >= rl.x0 && c.hi <= rl.x0 + rl.rw;
        }
    }
    for (int l = 0; l < NL; l++) {
        for (int k = 0; k < p.n_classes; k++) {
            const AxisKey &kr = keys[krow[k]], &kc = keys[kcol[k]];
            const RoiRect rl = d.rect_live[l][k];
            int *sh = d.rshare[l][k];
            sh[0] = sh[1] = sh[2] = sh[3] = 0;
            const int kk = l - 6 * bl;
            if (kk >= 0 && kk < 6 && takes[k]) {
                if (launched_rects(runs_of(kr.rc[kk]), runs_of(kc.rc[kk]), kk < 5, rl, f.rects[l][k], f.n[l][k])) f.any = true;
                std::copy(kr.rc[kk].begin(), kr.rc[kk].end(), mask_at(f.mask, ws, l, k, 0));
                std::copy(kc.rc[kk].begin(), kc.rc[kk].end(), mask_at(f.mask, ws, l, k, 1));
                if (kk == 5) {          // the copies: all of the bottleneck tensor's zone
                    sh[0] = kr.rshare.lo; sh[1] = kr.rshare.hi; sh[2] = kc.rshare.lo; sh[3] = kc.rshare.hi;
                    std::vector<Iv> rs, cs;
                    if (!empty(kr.rshare)) rs.push_back(kr.rshare);
                    if (!empty(kc.rshare)) cs.push_back(kc.rshare);
                    put_fills(f.fill, l, k, runs_of(kr.rc[5]), rs, runs_of(kc.rc[5]), cs);
                }
            } else {
                if (rl.rh > 0 && rl.rw > 0) f.rects[l][k][f.n[l][k]++] = rl;
                if (live_class(p, k)) {
                    const RoiRect lv = d.live[l][k];
                    std::fill_n(mask_at(f.mask, ws, l, k, 0) + lv.y0, lv.rh, (unsigned char)1);
                    std::fill_n(mask_at(f.mask, ws, l, k, 1) + lv.x0, lv.rw, (unsigned char)1);
                }
            }
        }
        tally(p, f, l);
    }
    if (!f.any) f.fill.clear();
}

// the exact sets in force below the fused levels' form: rcomp's in the unfused last level where the plan has that form, comp elsewhere
Mask masks_below_fused(const RoiDownPlan &d, int ws)
{
    Mask m = d.comp;
    const size_t per_layer = (size_t)ROI_MAX_CLASSES * 2 * ws, l0 = 6 * (size_t)(d.n_down - 1);
    if (d.rcomp.any) std::copy(d.rcomp.mask.begin() + l0 * per_layer, d.rcomp.mask.begin() + (l0 + 6) * per_layer, m.begin() + l0 * per_layer);
    return m;
}

// per class: the fused levels' rectangle launches in the shared-interior form and the halo strips of their pooled outputs
// (RoiDownPlan::fcomp); after share_rect_classes
void share_fused_rect_classes(RoiPlan &p, const std::vector<AxisKey> &keys, const int *krow, const int *kcol)
{
    RoiDownPlan &d = p.down;
    RectForm &f = d.fcomp;
    const int NL = d.n_layers, ws = p.ws, L = 6 * d.n_down;
    f = RectForm();
    for (int l = 0; l < NL; l++) d.fused_fill_on[l] = false;
    f.mask = masks_below_fused(d, ws);
    auto get = [&](int l, int k, int axis) { const unsigned char *m = mask_at(f.mask, ws, l, k, axis); return Mask(m, m + d.res[l]); };
    auto within = [](Mask a, Iv lv) { for (int i = 0; i < (int)a.size(); i++) a[i] = a[i] && in_iv(lv, i); return a; };
    const bool form = d.share_any && d.rcomp.any;
    auto in_form = [&](int b) { return form && b >= 0 && b < d.n_down && (((d.fused_mask & ROI_SHARE_LEVELS & ROI_SHARE_FUSED_RECT_LEVELS) >> b) & 1u); };
    bool takes[ROI_MAX_DOWN][ROI_MAX_CLASSES] = {};
    // the exact sets, from the deepest level upwards (the strips of level b read the sets of level b + 1)
    for (int b = d.n_down - 1; b >= 0; b--) {
        if (!in_form(b)) continue;
        const int l0 = 6 * b;
        const bool stem = b == 0 && (d.fused_mask & 1u);
        for (int k = 0; k < p.n_classes; k++) {
            const AxisKey &kr = keys[krow[k]], &kc = keys[kcol[k]];
            bool t = live_class(p, k) && (!empty(kr.share[l0 + 5]) || !empty(kc.share[l0 + 5]));
            Mask m[3][2];           // pooled output, residual, stem at the even pixels; rows, columns
            for (int ax = 0; ax < 2 && t; ax++) {
                const AxisKey &key = ax ? kc : kr;
                m[0][ax] = key.comp[l0 + 5];
                m[1][ax] = within(m[0][ax], key.live[l0 + 4]);
                m[2][ax] = stem ? within(m[1][ax], key.live[L]) : Mask();
                const int ls[3] = {l0 + 5, l0 + 4, L};
                for (int j = 0; j < (stem ? 3 : 2); j++) {
                    const RoiRect rl = d.rect_live[ls[j]][k];
                    const Iv box = ax ? Iv{rl.x0, rl.x0 + rl.rw} : Iv{rl.y0, rl.y0 + rl.rh};
                    const std::vector<Iv> runs = runs_of(m[j][ax]);
                    t = t && !runs.empty() && runs.size() <= 2;
                    for (const Iv &r : runs) t = t && r.lo >= box.lo && r.hi <= box.hi;
                }
            }
            takes[b][k] = t;
            if (!t) continue;
            for (int ax = 0; ax < 2; ax++) {
                std::copy(m[1][ax].begin(), m[1][ax].end(), mask_at(f.mask, ws, l0 + 4, k, ax));
                if (stem) std::copy(m[2][ax].begin(), m[2][ax].end(), mask_at(f.mask, ws, L, k, ax));
            }
        }
    }
    // the rectangles as launched, every layer: of the exact set where the class takes the form, rcomp's elsewhere
    for (int l = 0; l < NL; l++) {
        d.px_live[l] = d.copy_old[l] = d.copy_new[l] = 0;
        const int b = l == L ? 0 : l / 6, kk = l == L ? 4 : l % 6;
        const bool cut = l <= L && (kk == 4 || kk == 5) && (l != L || (d.fused_mask & 1u)) && in_form(b);
        for (int k = 0; k < p.n_classes; k++) {
            const RoiRect rl = d.rect_live[l][k];
            if (cut && takes[b][k]) {
                if (launched_rects(runs_of(get(l, k, 0)), runs_of(get(l, k, 1)), kk != 5, rl, f.rects[l][k], f.n[l][k])) f.any = true;
            } else {
                f.n[l][k] = d.rcomp.n[l][k];
                std::copy(d.rcomp.rects[l][k], d.rcomp.rects[l][k] + 4, f.rects[l][k]);
            }
            d.px_live[l] += (double)rl.rh * rl.rw * p.class_count[k];
        }
        tally(p, f, l);
    }
    // the halo strips of the pooled outputs: the shared pixels the next level's exact sets tap
    for (int b = 0; b + 1 < d.n_down; b++) {
        if (!in_form(b)) continue;
        const int l5 = 6 * b + 5, Ho = d.res[l5], ln = 6 * (b + 1);
        d.fused_fill_on[l5] = true;
        for (int k = 0; k < p.n_classes; k++) {
            if (!live_class(p, k)) continue;
            const AxisKey *key[2] = {&keys[krow[k]], &keys[kcol[k]]};
            std::vector<Iv> own[2], got[2];         // per axis: the tapped pixels the patch computes itself, and those in its shared zone
            for (int ax = 0; ax < 2; ax++) {
                const Mask dw = taps_of(get(ln, k, ax), TAP_DW, Ho), ev = taps_of(get(ln + 4, k, ax), TAP_EVEN, Ho);
                Mask o(Ho, 0), g(Ho, 0);
                for (int v = 0; v < Ho; v++) {
                    const bool tap = dw[v] || ev[v];
                    o[v] = tap && key[ax]->comp[l5][v];
                    g[v] = tap && in_iv(key[ax]->share[l5], v);
                }
                own[ax] = runs_of(o); got[ax] = runs_of(g);
            }
            put_fills(f.fill, l5, k, own[0], got[0], own[1], got[1]);
        }
        f.any = true;
    }
    // a table that does not fit keeps the form below, and so does a plan without the form: rcomp's tables, no strips
    if (!f.any || f.segs > ROI_MAX_SEGS - 1) {
        f = d.rcomp;
        f.any = false;
        f.fill.clear();
        f.mask = masks_below_fused(d, ws);
        for (int l = 0; l < NL; l++) d.fused_fill_on[l] = false;
    }
    // what is copied into a tensor without and with the form
    auto px_of = [&](const RoiDownPlan::ShareFill &c) { return (double)c.rh * c.rw * p.class_count[c.cls]; };
    for (const RoiDownPlan::ShareFill &c : f.fill) d.copy_new[c.layer] += px_of(c);
    for (const RoiDownPlan::ShareFill &c : d.share_fill) {
        d.copy_old[c.layer] += px_of(c);
        if (!d.fused_fill_on[c.layer]) d.copy_new[c.layer] += px_of(c);
    }
}

}  // namespace

void roi_plan_share(RoiPlan &p)
{
    RoiDownPlan &d = p.down;
    d.share_any = false;
    d.comp.clear(); d.share_fill.clear(); d.nbr.clear();
    if (d.n_down <= 0 || p.n_classes <= 0) return;
    const int ws = p.ws, n_down = d.n_down, NL = d.n_layers;
    const TileGeom g = make_geom(p.hh, p.ww, ws);
    if (g.tiles_per_img != p.tiles_per_img) return;
    // the ring: the same on both axes and for every class
    Iv inner[ROI_MAX_DOWN_LAYERS];
    inner_axis(ws, n_down, inner);
    for (int l = 0; l < NL; l++)
        for (int k = 0; k < p.n_classes; k++) d.inner[l][k] = rect_of(inner[l], inner[l]);
    // the axis keys, their successors and the neighbour map
    std::vector<AxisKey> keys;
    auto key_of = [&](Iv rd) -> int {
        for (int i = 0; i < (int)keys.size(); i++) if (keys[i].rd.lo == rd.lo && keys[i].rd.hi == rd.hi) return i;
        keys.emplace_back();
        keys.back().rd = rd;
        return (int)keys.size() - 1;
    };
    int krow[ROI_MAX_CLASSES], kcol[ROI_MAX_CLASSES];
    for (int k = 0; k < p.n_classes; k++) {
        const RoiRect &rd = p.read[k];
        krow[k] = key_of(Iv{rd.y0, rd.y0 + rd.rh});
        kcol[k] = key_of(Iv{rd.x0, rd.x0 + rd.rw});
    }
    d.nbr.assign((size_t)p.tiles_per_img * 3, -1);
    auto follow = [&](int key, int nxt) {
        if (nxt < 0) { keys[key].last = true; return; }
        if (std::find(keys[key].next.begin(), keys[key].next.end(), nxt) == keys[key].next.end()) keys[key].next.push_back(nxt);
    };
    for (int o = 0; o < 8; o++) {
        const int na = g.na[o & 1], nb = g.nb[o & 1];
        for (int a = 0; a < na; a++)
            for (int b = 0; b < nb; b++) {
                const int t = g.tile_off[o] + a * nb + b;
                const int tr = b + 1 < nb ? t + 1 : -1, tb = a + 1 < na ? t + nb : -1;
                d.nbr[3 * t] = tr; d.nbr[3 * t + 1] = tb; d.nbr[3 * t + 2] = (tr >= 0 && tb >= 0) ? t + nb + 1 : -1;
                follow(kcol[p.tile_class[t]], tr >= 0 ? kcol[p.tile_class[tr]] : -1);
                follow(krow[p.tile_class[t]], tb >= 0 ? krow[p.tile_class[tb]] : -1);
            }
    }
    // every key's live, and what it computes of its lower half whatever it shares itself
    const int L = 6 * n_down, R0 = ws >> p.n_up;
    for (AxisKey &key : keys) {
        if (empty(key.rd)) continue;
        Iv ur[ROI_MAX_LAYERS], uc[ROI_MAX_LAYERS], need[ROI_MAX_DOWN_LAYERS], rect[ROI_MAX_DOWN_LAYERS], nc[ROI_MAX_DOWN_LAYERS];
        Iv rl[ROI_MAX_DOWN_LAYERS], reads[ROI_MAX_DOWN_LAYERS];
        walk_back(key.rd, key.rd, ws, p.n_up, ur, uc, true);
        walk_down_axis(hull(ur[1], dilate(ur[0], 1, R0)), false, ws, n_down, d.fused_mask, need, rect);
        need[L + 3] = rect[L + 3] = key.rd;
        walk_const_axis(key.rd, false, ws, n_down, d.fused_mask, need, rect, nc, key.live, rl, reads);
    }
    auto shared_level = [&](int b) { return ((d.fused_mask & ROI_SHARE_LEVELS) >> b) & 1u; };
    for (AxisKey &key : keys)
        for (int b = 0; b < n_down; b++) {
            if (!shared_level(b)) continue;
            const int H = (ws / 2) >> b, Ho = H / 2;
            key.low[6 * b + 5] = mask_of(meet(key.live[6 * b + 5], Iv{0, Ho / 2}), Ho);
            const Mask t1 = taps_of(taps_of(key.low[6 * b + 5], TAP_S2, H), TAP_DW, H);
            Mask &lo1 = key.low[6 * b + 1];
            lo1.assign(H, 0);
            for (int v = 0; v < H / 2; v++) lo1[v] = t1[v] && in_iv(key.live[6 * b + 1], v);
        }
    // share, comp and the tiles of every key
    for (AxisKey &key : keys) {
        for (int l = 0; l < NL; l++) { key.comp[l] = mask_of(key.live[l], d.res[l]); key.sfill[l].assign(d.res[l], 0); key.tiles[l] = ~0ull; }
        if (key.last || key.next.empty() || empty(key.rd)) continue;
        for (int b = 0; b < n_down; b++) {
            if (!shared_level(b) || ((ws / 2) >> b) / 16 > 64) continue;
            const int H = (ws / 2) >> b, Ho = H / 2;
            // v of tensor l (side R) is shared when it is live and inner here, and v - R / 2 inner and computed in every successor
            auto zone = [&](int l, int R) {
                Mask m(R, 0);
                for (int v = R / 2; v < R; v++) {
                    bool ok = in_iv(key.live[l], v) && in_iv(inner[l], v) && in_iv(inner[l], v - R / 2);
                    for (size_t i = 0; ok && i < key.next.size(); i++) {
                        const Mask &lw = keys[key.next[i]].low[l];
                        ok = !lw.empty() && lw[v - R / 2];
                    }
                    m[v] = ok;
                }
                return longest_run(m);
            };
            const int l0 = 6 * b;
            key.share[l0 + 5] = zone(l0 + 5, Ho);
            key.share[l0 + 1] = zone(l0 + 1, H);
            if (empty(key.share[l0 + 5]) && empty(key.share[l0 + 1])) continue;
            Mask &c5 = key.comp[l0 + 5];
            for (int v = key.share[l0 + 5].lo; v < key.share[l0 + 5].hi; v++) c5[v] = 0;
            key.sfill[l0 + 5] = mask_of(key.share[l0 + 5], Ho);
            key.comp[l0 + 3] = key.comp[l0 + 2] = taps_of(c5, TAP_S2, H);
            const Mask t1 = taps_of(key.comp[l0 + 2], TAP_DW, H);
            Mask &c1 = key.comp[l0 + 1], &s1 = key.sfill[l0 + 1];
            for (int v = 0; v < H; v++) {
                const bool sh = in_iv(key.share[l0 + 1], v);
                c1[v] = t1[v] && in_iv(key.live[l0 + 1], v) && !sh;
                s1[v] = t1[v] && sh;
            }
            key.tiles[l0 + 3] = tiles_touching(key.comp[l0 + 3]);
            key.tiles[l0 + 1] = tiles_touching(c1);
            // a tapped shared pixel inside a tile that runs anyway is computed there, from the block's input, which is held whole: no copy
            for (int v = 0; v < H; v++)
                if (s1[v] && ((key.tiles[l0 + 1] >> (v / 16)) & 1ull)) { s1[v] = 0; c1[v] = 1; }
            key.comp[l0] = c1;
        }
    }
    share_rect_keys(p, keys, inner);
    // the classes: products of their two keys' sets
    d.comp.assign((size_t)NL * ROI_MAX_CLASSES * 2 * ws, 0);
    for (int k = 0; k < p.n_classes; k++) {
        const AxisKey &kr = keys[krow[k]], &kc = keys[kcol[k]];
        for (int l = 0; l < NL; l++) {
            int *sh = d.share[l][k];
            sh[0] = sh[1] = sh[2] = sh[3] = 0;
            d.tile_rows[l][k] = d.tile_cols[l][k] = ~0ull;
            if (!live_class(p, k)) continue;
            sh[0] = kr.share[l].lo; sh[1] = kr.share[l].hi; sh[2] = kc.share[l].lo; sh[3] = kc.share[l].hi;
            d.tile_rows[l][k] = kr.tiles[l]; d.tile_cols[l][k] = kc.tiles[l];
            std::copy(kr.comp[l].begin(), kr.comp[l].end(), mask_at(d.comp, ws, l, k, 0));
            std::copy(kc.comp[l].begin(), kc.comp[l].end(), mask_at(d.comp, ws, l, k, 1));
            if (!any(kr.sfill[l]) && !any(kc.sfill[l])) continue;
            d.share_any = true;
            put_fills(d.share_fill, l, k, runs_of(kr.comp[l]), runs_of(kr.sfill[l]), runs_of(kc.comp[l]), runs_of(kc.sfill[l]));
        }
    }
    share_rect_classes(p, keys, krow, kcol);
    share_fused_rect_classes(p, keys, krow, kcol);
}

void roi_share_neighbours(const RoiPlan &p, int k, std::vector<int> &out)
{
    const int T = p.tiles_per_img;
    out.assign((size_t)std::max(k, 0) * T * 3, -1);
    if ((int)p.down.nbr.size() != 3 * T) return;
    auto pos = [&](int img, int t) { const int c = p.tile_class[t]; return k * p.class_base[c] + img * p.class_count[c] + p.tile_rank[t]; };
    for (int img = 0; img < k; img++)
        for (int t = 0; t < T; t++)
            for (int j = 0; j < 3; j++)
                if (p.down.nbr[3 * t + j] >= 0) out[(size_t)3 * pos(img, t) + j] = pos(img, p.down.nbr[3 * t + j]);
}

// ---- what a pass launches under a form (roi_plan.h:RoiDownForm) ----
RoiDownForm roi_down_form(const RoiPlan &p, RoiDownForm want)
{
    const RoiDownPlan &d = p.down;
    RoiDownForm has = ROI_DOWN_FULL;
    if (p.n_classes > 0 && d.n_down > 0) has = ROI_DOWN_CONST;
    if (has == ROI_DOWN_CONST && d.share_any) has = ROI_DOWN_SHARE;
    if (has == ROI_DOWN_SHARE && d.rcomp.any && d.rcomp.segs + 1 <= ROI_MAX_SEGS) has = ROI_DOWN_SHARE_RECT;
    if (has == ROI_DOWN_SHARE_RECT && d.fcomp.any && d.fcomp.segs + 1 <= ROI_MAX_SEGS) has = ROI_DOWN_SHARE_FUSED_RECT;
    return std::min(has, want);
}

// the rectangles of one of the two rectangle forms (null: rect_live), the empty ones left out
static int form_rects(const RoiDownPlan &d, const RoiDownPlan::RectForm *f, int l, int k, RoiRect *out)
{
    if (f) {
        std::copy(f->rects[l][k], f->rects[l][k] + f->n[l][k], out);
        return f->n[l][k];
    }
    out[0] = d.rect_live[l][k];
    return out[0].rh > 0 && out[0].rw > 0 ? 1 : 0;
}

int roi_down_rects(const RoiPlan &p, RoiDownForm form, int l, int k, RoiRect out[4])
{
    const RoiDownPlan &d = p.down;
    switch (roi_down_form(p, form)) {
    case ROI_DOWN_FULL: return 0;
    case ROI_DOWN_REGION: out[0] = d.rect[l][k]; return out[0].rh > 0 && out[0].rw > 0 ? 1 : 0;
    case ROI_DOWN_SHARE_RECT: return form_rects(d, &d.rcomp, l, k, out);
    case ROI_DOWN_SHARE_FUSED_RECT: return form_rects(d, &d.fcomp, l, k, out);
    default: return form_rects(d, nullptr, l, k, out);
    }
}

int roi_down_stem_layer(const RoiPlan &p, RoiDownForm form)
{
    return roi_down_form(p, form) == ROI_DOWN_SHARE_FUSED_RECT ? 6 * p.down.n_down : 4;
}

long long roi_sep_tile_table(const RoiPlan &p, RoiDownForm form, int layer, int k, std::vector<int> &out)
{
    out.clear();
    const RoiDownPlan &d = p.down;
    form = roi_down_form(p, form);
    const int b = layer / 6, kk = layer % 6;
    if (form == ROI_DOWN_FULL || k < 1 || layer < 0 || b >= d.n_down || (kk != 1 && kk != 3) || !((d.fused_mask >> b) & 1u)) return 0;
    const bool share = form >= ROI_DOWN_SHARE;
    const int TW = d.res[layer] / 16, TPP = TW * TW;
    const long long full = (long long)k * p.tiles_per_img * TPP;
    if (full > 0x7fffffffLL || (share && TW > 64)) return 0;
    for (int cl = 0; cl < p.n_classes; cl++) {
        const RoiRect &q = (form == ROI_DOWN_REGION ? d.rect : d.rect_live)[layer][cl];         // whole tiles (a fused level's rectangles are rounded to 16)
        const int ty0 = q.y0 / 16, ty1 = (q.y0 + q.rh) / 16, tx0 = q.x0 / 16, tx1 = (q.x0 + q.rw) / 16;
        for (int pt = k * p.class_base[cl]; pt < k * p.class_base[cl + 1]; pt++)
            for (int ty = ty0; ty < ty1; ty++) {
                if (share && !((d.tile_rows[layer][cl] >> ty) & 1ull)) continue;
                for (int tx = tx0; tx < tx1; tx++)
                    if (!share || ((d.tile_cols[layer][cl] >> tx) & 1ull)) out.push_back(pt * TPP + ty * TW + tx);
            }
    }
    return full;
}

// the quadrant table of fused layer 6 b + kk (kk = 1: roi_sep_quad_table, 3: roi_sep_quad_pool_table) -- one rule, one order
static long long sep_quad_table(const RoiPlan &p, RoiDownForm form, int layer, int kk, int k, std::vector<int> &out, long long *n_own, long long *n_ids)
{
    out.clear();
    *n_own = *n_ids = 0;
    const RoiDownPlan &d = p.down;
    // (asked for the shared-interior form or above: a plan in which no class shares resolves it to the constant-ring form, whose comp is live)
    if (form < ROI_DOWN_SHARE || roi_down_form(p, form) < ROI_DOWN_CONST || layer < 0 || layer % 6 != kk || d.comp.empty()) return 0;
    form = roi_down_form(p, form);
    std::vector<int> tiles;
    const long long full = roi_sep_tile_table(p, form, layer, k, tiles);
    if (full <= 0) return 0;
    const int TW = d.res[layer] / 16, TPP = TW * TW, QW = 2 * TW, QPP = QW * QW;
    if (((long long)k * p.tiles_per_img + k) * QPP > 0x7fffffffLL) return 0;
    // the class of a patch of the pass's class-major order
    std::vector<int> cls_of((size_t)k * p.tiles_per_img, 0);
    for (int cl = 0; cl < p.n_classes; cl++)
        for (int pt = k * p.class_base[cl]; pt < k * p.class_base[cl + 1]; pt++) cls_of[pt] = cl;
    auto holds = [&](int cl, int axis, int q) {         // does quadrant row / column q hold a comp row / column of the class?
        const unsigned char *m = d.comp.data() + (((size_t)layer * ROI_MAX_CLASSES + cl) * 2 + axis) * p.ws + 8 * q;
        return std::any_of(m, m + 8, [](unsigned char v) { return v != 0; });
    };
    for (int id : tiles) {
        const int pt = id / TPP, tr = id % TPP, ty = tr / TW, tx = tr % TW, cl = cls_of[pt];
        for (int qy = 2 * ty; qy < 2 * ty + 2; qy++)
            for (int qx = 2 * tx; qx < 2 * tx + 2; qx++)
                if (holds(cl, 0, qy) && holds(cl, 1, qx)) out.push_back(pt * QPP + qy * QW + qx);
    }
    *n_own = (long long)out.size();
    for (int pt = k * p.tiles_per_img; pt < k * p.tiles_per_img + k; pt++)      // tile by tile: a whole tile comes out as itself
        for (int tr = 0; tr < TPP; tr++)
            for (int s = 0; s < 4; s++) out.push_back(pt * QPP + (2 * (tr / TW) + (s >> 1)) * QW + 2 * (tr % TW) + (s & 1));
    *n_ids = (long long)out.size();
    while (out.size() % 4) out.push_back(out.back());
    return full;
}

long long roi_sep_quad_table(const RoiPlan &p, RoiDownForm form, int layer, int k, std::vector<int> &out, long long *n_own, long long *n_ids)
{
    return sep_quad_table(p, form, layer, 1, k, out, n_own, n_ids);
}

long long roi_sep_quad_pool_table(const RoiPlan &p, RoiDownForm form, int layer, int k, std::vector<int> &out, long long *n_own, long long *n_ids)
{
    return sep_quad_table(p, form, layer, 3, k, out, n_own, n_ids);
}

void roi_down_segs(const RoiPlan &p, RoiDownForm form, int l, int k, RoiSegs &out)
{
    out = RoiSegs{};
    form = roi_down_form(p, form);
    for (int cl = 0; cl < p.n_classes; cl++) {
        RoiRect q[4];
        const int nq = p.class_count[cl] > 0 ? roi_down_rects(p, form, l, cl, q) : 0;
        for (int i = 0; i < nq; i++) {
            RoiSeg &g = out.s[out.nseg++];
            g.p0 = k * p.class_base[cl]; g.np = k * p.class_count[cl];
            g.y0 = q[i].y0; g.x0 = q[i].x0; g.rh = q[i].rh; g.rw = q[i].rw;
        }
    }
    if (form >= ROI_DOWN_CONST) {
        RoiSeg &g = out.s[out.nseg++];
        g.p0 = k * p.tiles_per_img; g.np = k; g.rh = g.rw = p.down.res[l];
    }
}

void roi_down_const_items(const RoiPlan &p, RoiDownForm form, int l, int k, FillItems &out)
{
    out = FillItems{};
    if (roi_down_form(p, form) < ROI_DOWN_CONST) return;
    for (int cl = 0; cl < p.n_classes; cl++)
        for (int i = 0; i < 4 && p.class_count[cl] > 0; i++) {
            const RoiRect &q = p.down.fill[l][cl][i];
            if (q.rh <= 0 || q.rw <= 0) continue;
            out.it[out.n++] = FillItem{k * p.class_base[cl], k * p.class_count[cl], p.class_count[cl], q.y0, q.x0, q.rh, q.rw};
        }
}

void roi_down_copy_items(const RoiPlan &p, RoiDownForm form, int l, int k, std::vector<ShareItem> &out)
{
    out.clear();
    const RoiDownPlan &d = p.down;
    form = roi_down_form(p, form);
    if (form < ROI_DOWN_SHARE) return;
    auto take = [&](const std::vector<RoiDownPlan::ShareFill> &from) {
        for (const RoiDownPlan::ShareFill &f : from)
            if (f.layer == l) out.push_back(ShareItem{k * p.class_base[f.cls], k * p.class_count[f.cls], f.dir, f.y0, f.x0, f.rh, f.rw});
    };
    take(form == ROI_DOWN_SHARE_FUSED_RECT && d.fused_fill_on[l] ? d.fcomp.fill : d.share_fill);
    if (form >= ROI_DOWN_SHARE_RECT) take(d.rcomp.fill);
}

bool roi_make_plan(int hh, int ww, int ws, int n_up, const int *chan, int max_classes, RoiPlan &out)
{
    out = RoiPlan();
    if (hh < 1 || ww < 1 || ws < 1 || n_up < 1 || n_up > ROI_MAX_UP || !chan || (ws % (4 << n_up)) != 0) return false;
    max_classes = std::min(max_classes, ROI_MAX_CLASSES);
    const TileGeom g = make_geom(hh, ww, ws);
    out.hh = hh; out.ww = ww; out.ws = ws; out.n_up = n_up;
    out.tiles_per_img = g.tiles_per_img;
    out.n_layers = 3 * n_up + 1;
    for (int j = 0, R = ws >> n_up; j < n_up; j++) {
        out.res[3 * j] = out.res[3 * j + 1] = R;
        if (j) R *= 2;
        out.res[3 * j + 2] = R;
    }
    out.res[3 * n_up] = ws / 2;
    double mpp[ROI_MAX_LAYERS];             // multiply-accumulates per enumerated pixel
    for (int j = 0; j < n_up; j++) {
        mpp[3 * j] = (j ? 16.0 : 9.0) * chan[j] * chan[j + 1];
        mpp[3 * j + 1] = 1.0 * chan[j] * chan[j + 1];
        mpp[3 * j + 2] = 9.0 * chan[j + 1] * chan[j + 1];
    }
    mpp[3 * n_up] = 16.0 * chan[n_up];
    for (int l = 0; l < out.n_layers; l++) out.mac_full[l] = mpp[l] * out.res[l] * out.res[l] * g.tiles_per_img;

    // classes: the rectangle (patch ∩ interior) of every tile, in the order of first appearance
    struct Key { Iv r, c; };
    std::vector<Key> keys;
    out.tile_class.assign(g.tiles_per_img, 0);
    out.tile_rank.assign(g.tiles_per_img, 0);
    bool fallback = false;
    for (int o = 0; o < 8 && !fallback; o++) {
        const int FH = (o & 1) ? g.Wp : g.Hp, FW = (o & 1) ? g.Hp : g.Wp;
        const int na = g.na[o & 1], nb = g.nb[o & 1];
        for (int a = 0; a < na && !fallback; a++)
            for (int b = 0; b < nb; b++) {
                Iv r = clip(Iv{g.aug - a * g.step, FH - g.aug - a * g.step}, ws), c = clip(Iv{g.aug - b * g.step, FW - g.aug - b * g.step}, ws);
                if (r.hi <= r.lo || c.hi <= c.lo) r = c = Iv{0, 0};
                int k = 0;
                for (; k < (int)keys.size(); k++)
                    if (keys[k].r.lo == r.lo && keys[k].r.hi == r.hi && keys[k].c.lo == c.lo && keys[k].c.hi == c.hi) break;
                if (k == (int)keys.size()) {
                    if (k == max_classes) { fallback = true; break; }
                    keys.push_back(Key{r, c});
                }
                const int tile = g.tile_off[o] + a * nb + b;
                out.tile_class[tile] = k;
                out.tile_rank[tile] = out.class_count[k]++;
            }
    }
    if (fallback) {         // too many classes: no plan, every launch full-frame
        std::fill(out.tile_class.begin(), out.tile_class.end(), 0);
        for (int t = 0; t < g.tiles_per_img; t++) out.tile_rank[t] = t;
        std::fill(out.class_count, out.class_count + ROI_MAX_CLASSES, 0);
        for (int l = 0; l < out.n_layers; l++) out.mac_planned[l] = out.mac_planned_tight[l] = out.mac_planned_exact[l] = out.mac_full[l];
        return true;
    }
    out.n_classes = (int)keys.size();
    for (int k = 0; k < out.n_classes; k++) out.class_base[k + 1] = out.class_base[k] + out.class_count[k];
    for (int k = 0; k < out.n_classes; k++) {
        Iv rows[ROI_MAX_LAYERS], cols[ROI_MAX_LAYERS];
        const bool empty = keys[k].r.hi <= keys[k].r.lo;
        out.read[k] = RoiRect{keys[k].r.lo, keys[k].c.lo, keys[k].r.hi - keys[k].r.lo, keys[k].c.hi - keys[k].c.lo};
        if (!empty) walk_back(keys[k].r, keys[k].c, ws, n_up, rows, cols);
        for (int l = 0; l < out.n_layers; l++) {
            RoiRect q{0, 0, 0, 0};
            if (!empty) q = RoiRect{rows[l].lo, cols[l].lo, rows[l].hi - rows[l].lo, cols[l].hi - cols[l].lo};
            out.rect[l][k] = q;
            out.mac_planned[l] += mpp[l] * q.rh * q.rw * out.class_count[k];
        }
        // The tight form: every layer rounds ITS OWN need -- the exact walk, as the down plan does (roi_plan_down) -- instead of growing
        // from its consumer's rounded rectangle, whose extra columns would otherwise be rounded again in every producer.  Rows are never
        // rounded.  The final convolution keeps its whole 8 x 16 blocks.
        Iv er[ROI_MAX_LAYERS], ec[ROI_MAX_LAYERS];
        if (!empty) walk_back(keys[k].r, keys[k].c, ws, n_up, er, ec, true);
        Iv xr[ROI_MAX_LAYERS], xc[ROI_MAX_LAYERS];          // the need with the sub-pixel layers' parity: the exact rectangles
        if (!empty) walk_back(keys[k].r, keys[k].c, ws, n_up, xr, xc, true, true);
        for (int l = 0; l < out.n_layers; l++) {
            RoiRect q = out.rect[l][k];
            if (!empty && l + 1 < out.n_layers) {
                const Iv c = align_cols_in(ec[l], out.res[l], cols[l]);
                q = RoiRect{er[l].lo, c.lo, er[l].hi - er[l].lo, c.hi - c.lo};
            }
            out.rect_tight[l][k] = q;
            out.mac_planned_tight[l] += mpp[l] * q.rh * q.rw * out.class_count[k];
            // The exact form: the need itself (conv_mfma_kernel<..., ROI> takes any first column and any width)
            if (!empty && l + 1 < out.n_layers && !((ROI_EXACT_KEEP_TIGHT >> l) & 1u))
                q = RoiRect{xr[l].lo, xc[l].lo, xr[l].hi - xr[l].lo, xc[l].hi - xc[l].lo};
            out.rect_exact[l][k] = q;
            out.mac_planned_exact[l] += mpp[l] * q.rh * q.rw * out.class_count[k];
        }
    }
    return true;
}

}  // namespace tmat

using namespace tmat;

static int roi_plan_export(int set, int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                           int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full)
{
    if (!channels || !tiles_per_img || !n_classes || !tile_class || !tile_rank || !class_count || !rects || !mac_planned || !mac_full ||
        max_classes < 1 || max_classes > ROI_MAX_CLASSES) {
        set_error("tmat_roi_plan: bad argument");
        return TMAT_E_ARG;
    }
    RoiPlan p;
    if (!roi_make_plan(hh, ww, patch, n_up, channels, max_classes, p)) { set_error("tmat_roi_plan: unsupported geometry"); return TMAT_E_ARG; }
    *tiles_per_img = p.tiles_per_img;
    if (p.tiles_per_img > tiles_cap) { set_error("tmat_roi_plan: tiles_cap too small"); return TMAT_E_ARG; }
    *n_classes = p.n_classes;
    for (int t = 0; t < p.tiles_per_img; t++) { tile_class[t] = p.tile_class[t]; tile_rank[t] = p.tile_rank[t]; }
    for (int k = 0; k < max_classes; k++) class_count[k] = k < p.n_classes ? p.class_count[k] : 0;
    for (int l = 0; l < p.n_layers; l++) {
        for (int k = 0; k < max_classes; k++) {
            const RoiRect q = k < p.n_classes ? (set == 2 ? p.rect_exact : set == 1 ? p.rect_tight : p.rect)[l][k] : RoiRect{0, 0, 0, 0};
            int *o = rects + ((size_t)l * max_classes + k) * 4;
            o[0] = q.y0; o[1] = q.x0; o[2] = q.rh; o[3] = q.rw;
        }
        mac_planned[l] = set == 2 ? p.mac_planned_exact[l] : set == 1 ? p.mac_planned_tight[l] : p.mac_planned[l];
        mac_full[l] = p.mac_full[l];
    }
    return TMAT_OK;
}

// the nested rectangles (what TMAT_ROI_TIGHT=0 launches), whatever the environment says
extern "C" int tmat_roi_plan(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                             int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full)
{
    return roi_plan_export(0, hh, ww, patch, n_up, channels, max_classes, tiles_cap, tiles_per_img, n_classes, tile_class, tile_rank,
                           class_count, rects, mac_planned, mac_full);
}

// the same plan with the tight rectangles (what TMAT_ROI_EXACT=0 launches)
extern "C" int tmat_roi_plan_tight(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                                   int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full)
{
    return roi_plan_export(1, hh, ww, patch, n_up, channels, max_classes, tiles_cap, tiles_per_img, n_classes, tile_class, tile_rank,
                           class_count, rects, mac_planned, mac_full);
}

// the same plan with the exact rectangles (the default of the tiled entry points)
extern "C" int tmat_roi_plan_exact(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
                                   int *n_classes, int *tile_class, int *tile_rank, int *class_count, int *rects, double *mac_planned, double *mac_full)
{
    return roi_plan_export(2, hh, ww, patch, n_up, channels, max_classes, tiles_cap, tiles_per_img, n_classes, tile_class, tile_rank,
                           class_count, rects, mac_planned, mac_full);
}

// ---- the exports of the down plan: what they share ----
// the argument check (args_ok: the export's own pointers and caps) and the plan; TMAT_OK, or the error set under the export's name
static int down_plan_for(const char *name, bool args_ok, int hh, int ww, int patch, int n_up, const int *up_channels, int n_down,
                         const int *down_channels, unsigned fused_mask, int max_classes, RoiPlan &p)
{
    if (!args_ok || !up_channels || !down_channels || max_classes < 1 || max_classes > ROI_MAX_CLASSES) {
        set_error(std::string(name) + ": bad argument");
        return TMAT_E_ARG;
    }
    if (!roi_make_plan(hh, ww, patch, n_up, up_channels, max_classes, p) || !roi_plan_down(p, n_down, down_channels, fused_mask)) {
        set_error(std::string(name) + ": unsupported geometry");
        return TMAT_E_ARG;
    }
    return TMAT_OK;
}
// a rectangle as (y0, x0, rows, columns); `in` false: a class the plan does not have, zeros
static void put_rect(int *o, const RoiRect &q, bool in = true)
{
    o[0] = in ? q.y0 : 0; o[1] = in ? q.x0 : 0; o[2] = in ? q.rh : 0; o[3] = in ? q.rw : 0;
}
// [max_classes][4 rectangles][4] and their counts for layer l: the rectangles of form f (null: rect_live)
static void put_form_rects(const RoiPlan &p, const RoiDownPlan::RectForm *f, int l, int max_classes, int *n_rects, int *rects)
{
    for (int k = 0; k < max_classes; k++) {
        RoiRect q[4] = {};
        const int n = k < p.n_classes ? form_rects(p.down, f, l, k, q) : 0;
        n_rects[(size_t)l * max_classes + k] = n;
        for (int i = 0; i < 4; i++) put_rect(rects + (((size_t)l * max_classes + k) * 4 + i) * 4, q[i], i < n);
    }
}
// [max_classes][2 axes][patch] bytes for layer l out of a table in the layout of RoiDownPlan::comp (empty: zeros)
static void put_masks(const RoiPlan &p, const std::vector<unsigned char> &m, int l, int max_classes, unsigned char *comp)
{
    for (int k = 0; k < max_classes; k++) {
        unsigned char *o = comp + ((size_t)l * max_classes + k) * 2 * p.ws;
        if (k < p.n_classes && !m.empty()) std::copy_n(m.data() + ((size_t)l * ROI_MAX_CLASSES + k) * 2 * p.ws, 2 * p.ws, o);
        else std::fill_n(o, 2 * p.ws, (unsigned char)0);
    }
}
// [n_fill][7] as (layer, class, direction, y0, x0, rows, columns)
static int put_fill_list(const char *name, const std::vector<RoiDownPlan::ShareFill> &v, int fill_cap, int *n_fill, int *fills)
{
    *n_fill = (int)v.size();
    if (*n_fill > fill_cap) { set_error(std::string(name) + ": fill_cap too small"); return TMAT_E_ARG; }
    for (size_t i = 0; i < v.size(); i++) {
        const int o[7] = {v[i].layer, v[i].cls, v[i].dir, v[i].y0, v[i].x0, v[i].rh, v[i].rw};
        std::copy(o, o + 7, fills + i * 7);
    }
    return TMAT_OK;
}

// The down-path tables of the same plan (roi_plan_down): rects and needs [6 n_down + 4][max_classes][4] as (y0, x0, rows, columns),
// the four per-layer totals [6 n_down + 4], free_tile [n_down].  down_channels: n_down + 1 entries, the stem's first.
extern "C" int tmat_roi_plan_down(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                  unsigned fused_mask, int max_classes, int *n_classes, int *rects, int *needs, double *mac_planned,
                                  double *mac_full, double *bytes_planned, double *bytes_full, int *free_tile)
{
    RoiPlan p;
    const bool args_ok = n_classes && rects && needs && mac_planned && mac_full && bytes_planned && bytes_full && free_tile;
    if (int rc = down_plan_for("tmat_roi_plan_down", args_ok, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, max_classes, p)) return rc;
    *n_classes = p.n_classes;
    const RoiDownPlan &d = p.down;
    for (int l = 0; l < d.n_layers; l++) {
        for (int k = 0; k < max_classes; k++) {
            const size_t at = ((size_t)l * max_classes + k) * 4;
            put_rect(rects + at, d.rect[l][k], k < p.n_classes);
            put_rect(needs + at, d.need[l][k], k < p.n_classes);
        }
        mac_planned[l] = d.mac_planned[l]; mac_full[l] = d.mac_full[l];
        bytes_planned[l] = d.bytes_planned[l]; bytes_full[l] = d.bytes_full[l];
    }
    for (int b = 0; b < d.n_down; b++) free_tile[b] = d.free_tile[b] ? 1 : 0;
    return TMAT_OK;
}

// The tile table of a fused separable layer of the same plan for a pass of k images (roi_sep_tile_table): *n_full the full-frame tile
// count, *n_tiles the planned one; tiles (nullable: counts only) takes the planned tiles' full-frame ids, cap its room.
static int sep_tiles_export(RoiDownForm form, int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                            unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles)
{
    RoiPlan p;
    if (int rc = down_plan_for("tmat_roi_sep_tiles", n_tiles && n_full && k >= 1, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask,
                               ROI_MAX_CLASSES, p)) return rc;
    std::vector<int> tab;
    const long long full = roi_sep_tile_table(p, form, layer, k, tab);
    if (full <= 0) { set_error("tmat_roi_sep_tiles: not a fused separable layer of the plan"); return TMAT_E_ARG; }
    *n_full = (int)full;
    *n_tiles = (int)tab.size();
    if (tiles) {
        if ((int)tab.size() > cap) { set_error("tmat_roi_sep_tiles: cap too small"); return TMAT_E_ARG; }
        std::copy(tab.begin(), tab.end(), tiles);
    }
    return TMAT_OK;
}

// the tiles of ROI_DOWN_REGION
extern "C" int tmat_roi_sep_tiles(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                  unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles)
{
    return sep_tiles_export(ROI_DOWN_REGION, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, layer, k, cap, n_tiles, n_full, tiles);
}

// the same of ROI_DOWN_CONST: the tiles of rect_live, a subsequence of tmat_roi_sep_tiles' table
extern "C" int tmat_roi_sep_tiles_live(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                       unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles)
{
    return sep_tiles_export(ROI_DOWN_CONST, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, layer, k, cap, n_tiles, n_full, tiles);
}

// the same of ROI_DOWN_SHARE: a subsequence of tmat_roi_sep_tiles_live's table, in its order
extern "C" int tmat_roi_sep_tiles_share(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                        unsigned fused_mask, int layer, int k, int cap, int *n_tiles, int *n_full, int *tiles)
{
    return sep_tiles_export(ROI_DOWN_SHARE, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, layer, k, cap, n_tiles, n_full, tiles);
}

// The quadrant table of plain fused layer 6 b + 1 of the same plan for a pass of k images under `form` (roi_sep_quad_table; refused below
// ROI_DOWN_SHARE and for every other layer).  counts[4]: the table's length (a multiple of 4: the packed tiles x 4), the ids of the
// pass's own patches, all ids before the padding, the full-frame tile count of the pass's own patches.  ids (nullable: counts only)
// takes the table, cap its room.
extern "C" int tmat_roi_sep_quads(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                  unsigned fused_mask, int form, int layer, int k, int cap, int *counts, int *ids)
{
    RoiPlan p;
    if (int rc = down_plan_for("tmat_roi_sep_quads", counts && k >= 1 && form >= ROI_DOWN_FULL && form <= ROI_DOWN_SHARE_FUSED_RECT, hh, ww, patch, n_up,
                               up_channels, n_down, down_channels, fused_mask, ROI_MAX_CLASSES, p)) return rc;
    std::vector<int> tab;
    long long n_own = 0, n_ids = 0;
    const long long full = roi_sep_quad_table(p, (RoiDownForm)form, layer, k, tab, &n_own, &n_ids);
    if (full <= 0) { set_error("tmat_roi_sep_quads: not a plain fused layer of the plan under a sharing form"); return TMAT_E_ARG; }
    counts[0] = (int)tab.size(); counts[1] = (int)n_own; counts[2] = (int)n_ids; counts[3] = (int)full;
    if (ids) {
        if ((int)tab.size() > cap) { set_error("tmat_roi_sep_quads: cap too small"); return TMAT_E_ARG; }
        std::copy(tab.begin(), tab.end(), ids);
    }
    return TMAT_OK;
}

// The same of pooled fused layer 6 b + 3 (roi_sep_quad_pool_table; refused below ROI_DOWN_SHARE and for every other layer): same counts
extern "C" int tmat_roi_sep_quads_pool(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                       unsigned fused_mask, int form, int layer, int k, int cap, int *counts, int *ids)
{
    RoiPlan p;
    if (int rc = down_plan_for("tmat_roi_sep_quads_pool", counts && k >= 1 && form >= ROI_DOWN_FULL && form <= ROI_DOWN_SHARE_FUSED_RECT, hh, ww, patch,
                               n_up, up_channels, n_down, down_channels, fused_mask, ROI_MAX_CLASSES, p)) return rc;
    std::vector<int> tab;
    long long n_own = 0, n_ids = 0;
    const long long full = roi_sep_quad_pool_table(p, (RoiDownForm)form, layer, k, tab, &n_own, &n_ids);
    if (full <= 0) { set_error("tmat_roi_sep_quads_pool: not a pooled fused layer of the plan under a sharing form"); return TMAT_E_ARG; }
    counts[0] = (int)tab.size(); counts[1] = (int)n_own; counts[2] = (int)n_ids; counts[3] = (int)full;
    if (ids) {
        if ((int)tab.size() > cap) { set_error("tmat_roi_sep_quads_pool: cap too small"); return TMAT_E_ARG; }
        std::copy(tab.begin(), tab.end(), ids);
    }
    return TMAT_OK;
}

// The constant-ring tables of the same plan (RoiDownPlan::nonconst ...): nonconst, live and rect_live [6 n_down + 4][max_classes][4] as
// (y0, x0, rows, columns), fill [6 n_down + 4][max_classes][4 strips][4], stored [6 n_down + 4], the two per-layer totals of rect_live.
extern "C" int tmat_roi_plan_const(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                   unsigned fused_mask, int max_classes, int *n_classes, int *nonconst, int *live, int *rect_live, int *fill,
                                   int *stored, double *mac_live, double *bytes_live)
{
    RoiPlan p;
    const bool args_ok = n_classes && nonconst && live && rect_live && fill && stored && mac_live && bytes_live;
    if (int rc = down_plan_for("tmat_roi_plan_const", args_ok, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, max_classes, p)) return rc;
    *n_classes = p.n_classes;
    const RoiDownPlan &d = p.down;
    for (int l = 0; l < d.n_layers; l++) {
        for (int k = 0; k < max_classes; k++) {
            const bool in = k < p.n_classes;
            const size_t at = ((size_t)l * max_classes + k) * 4;
            put_rect(nonconst + at, d.nonconst[l][k], in);
            put_rect(live + at, d.live[l][k], in);
            put_rect(rect_live + at, d.rect_live[l][k], in);
            for (int i = 0; i < 4; i++) put_rect(fill + (at + i) * 4, d.fill[l][k][i], in);
        }
        stored[l] = d.stored[l] ? 1 : 0;
        mac_live[l] = d.mac_live[l]; bytes_live[l] = d.bytes_live[l];
    }
    return TMAT_OK;
}

// The shared-interior tables of the same plan (RoiDownPlan::inner ...): inner [6 n_down + 4][max_classes][4] as (y0, x0, rows, columns),
// share [6 n_down + 4][max_classes][4] as (row lo, row hi, column lo, column hi), comp [6 n_down + 4][max_classes][2 axes][patch] bytes,
// fills [n_fill][7] as (layer, class, direction, y0, x0, rows, columns), neighbours [tiles_per_img][3] image-major tiles or -1.
extern "C" int tmat_roi_plan_share(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                   unsigned fused_mask, int max_classes, int *n_classes, int *inner, int *share, unsigned char *comp,
                                   int fill_cap, int *n_fill, int *fills, int tiles_cap, int *neighbours)
{
    RoiPlan p;
    const bool args_ok = n_classes && inner && share && comp && n_fill && fills && neighbours && fill_cap >= 0;
    if (int rc = down_plan_for("tmat_roi_plan_share", args_ok, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, max_classes, p)) return rc;
    const RoiDownPlan &d = p.down;
    if (p.tiles_per_img > tiles_cap || (int)d.nbr.size() != 3 * p.tiles_per_img) { set_error("tmat_roi_plan_share: tiles_cap too small"); return TMAT_E_ARG; }
    *n_classes = p.n_classes;
    for (int l = 0; l < d.n_layers; l++) {
        for (int k = 0; k < max_classes; k++) {
            const size_t at = ((size_t)l * max_classes + k) * 4;
            put_rect(inner + at, d.inner[l][k], k < p.n_classes);
            for (int i = 0; i < 4; i++) share[at + i] = k < p.n_classes ? d.share[l][k][i] : 0;
        }
        put_masks(p, d.comp, l, max_classes, comp);
    }
    std::copy(d.nbr.begin(), d.nbr.end(), neighbours);
    return put_fill_list("tmat_roi_plan_share", d.share_fill, fill_cap, n_fill, fills);
}

// The rectangle launches' shared-interior tables of the same plan (RoiDownPlan::rcomp ...): share [6 n_down + 4][max_classes][4] as (row
// lo, row hi, column lo, column hi), n_rects [6 n_down + 4][max_classes], rects [6 n_down + 4][max_classes][4 rectangles][4] as (y0, x0,
// rows, columns), comp [6 n_down + 4][max_classes][2 axes][patch] bytes (the exact sets, before the columns are rounded), fills [n_fill][7]
// as (layer, class, direction, y0, x0, rows, columns), the planned multiply-accumulates and bytes per layer, info: (some class differs
// from rect_live, the level that takes the form or -1, the longest segment table of a launch).
extern "C" int tmat_roi_plan_share_rect(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                        unsigned fused_mask, int max_classes, int *n_classes, int *share, int *n_rects, int *rects,
                                        unsigned char *comp, int fill_cap, int *n_fill, int *fills, double *mac_rect, double *bytes_rect, int *info)
{
    RoiPlan p;
    const bool args_ok = n_classes && share && n_rects && rects && comp && n_fill && fills && mac_rect && bytes_rect && info && fill_cap >= 0;
    if (int rc = down_plan_for("tmat_roi_plan_share_rect", args_ok, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, max_classes, p)) return rc;
    const RoiDownPlan &d = p.down;
    const RoiDownPlan::RectForm &f = d.rcomp;
    *n_classes = p.n_classes;
    for (int l = 0; l < d.n_layers; l++) {
        put_form_rects(p, f.any ? &f : nullptr, l, max_classes, n_rects, rects);
        put_masks(p, f.mask, l, max_classes, comp);
        for (int k = 0; k < max_classes; k++)
            for (int i = 0; i < 4; i++) share[((size_t)l * max_classes + k) * 4 + i] = k < p.n_classes ? d.rshare[l][k][i] : 0;
        mac_rect[l] = f.mask.empty() ? d.mac_live[l] : f.mac[l];
        bytes_rect[l] = f.mask.empty() ? d.bytes_live[l] : f.bytes[l];
    }
    info[0] = f.any ? 1 : 0;
    info[1] = f.any ? d.n_down - 1 : -1;
    info[2] = f.segs;
    return put_fill_list("tmat_roi_plan_share_rect", f.fill, fill_cap, n_fill, fills);
}

// The same for the fused levels' rectangle launches (RoiDownPlan::fcomp ...): n_rects [6 n_down + 4][max_classes], rects [6 n_down + 4]
// [max_classes][4 rectangles][4] as (y0, x0, rows, columns), comp [6 n_down + 4][max_classes][2 axes][patch] bytes (the exact sets in
// force, before the columns are rounded), fills [n_fill][7] as (layer, class, direction, y0, x0, rows, columns): the halo strips, fill_on
// [6 n_down + 4]: the strips stand in place of the layer's items of tmat_roi_plan_share, totals [6 n_down + 4][6]: planned
// multiply-accumulates, planned bytes, planned pixels, pixels of rect_live, copied pixels without and with the form (all per image),
// info: (some table differs from tmat_roi_plan_share_rect's, the mask of levels in force, the longest segment table of a launch).
extern "C" int tmat_roi_plan_share_fused_rect(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                              unsigned fused_mask, int max_classes, int *n_classes, int *n_rects, int *rects, unsigned char *comp,
                                              int fill_cap, int *n_fill, int *fills, int *fill_on, double *totals, int *info)
{
    RoiPlan p;
    const bool args_ok = n_classes && n_rects && rects && comp && n_fill && fills && fill_on && totals && info && fill_cap >= 0;
    if (int rc = down_plan_for("tmat_roi_plan_share_fused_rect", args_ok, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, max_classes, p))
        return rc;
    const RoiDownPlan &d = p.down;
    const RoiDownPlan::RectForm &f = d.fcomp;
    *n_classes = p.n_classes;
    unsigned levels = 0;
    for (int l = 0; l < d.n_layers; l++) {
        put_form_rects(p, f.any ? &f : d.rcomp.any ? &d.rcomp : nullptr, l, max_classes, n_rects, rects);
        put_masks(p, f.mask, l, max_classes, comp);
        fill_on[l] = d.fused_fill_on[l] ? 1 : 0;
        if (d.fused_fill_on[l]) levels |= 1u << (l / 6);
        const double t[6] = {f.mask.empty() ? d.mac_live[l] : f.mac[l], f.mask.empty() ? d.bytes_live[l] : f.bytes[l], f.px[l], d.px_live[l],
                             d.copy_old[l], d.copy_new[l]};
        std::copy(t, t + 6, totals + (size_t)l * 6);
    }
    info[0] = f.any ? 1 : 0;
    info[1] = (int)levels;
    info[2] = f.segs;
    return put_fill_list("tmat_roi_plan_share_fused_rect", f.fill, fill_cap, n_fill, fills);
}

// What a pass of k images launches under `form` (a RoiDownForm from ROI_DOWN_REGION upwards; roi_plan.h has the rule), as the planner
// hands it to the launches.  info: (the form the plan runs -- the one asked for or the highest below it that the plan has --, the
// layer whose table the stem at the even pixels launches, the longest segment table, all segment tables of the pass's rectangle
// launches added up: stem at the even pixels where level 0 is fused, residual and fix-up of a fused level, all six layers of an unfused
// one).  Per layer of the down plan: n_segs [6 n_down + 4] and segs [6 n_down + 4][64][6] as (p0, np, y0, x0, rows, columns) in launch
// order, the constant patches' segment included.  const_fills [n_const][7] as (layer, p0, np, y0, x0, rows, columns): the strips out
// of the constant patches.  copies [n_copy][8] as (layer, p0, np, direction, y0, x0, rows, columns): the neighbour items, in launch order.
extern "C" int tmat_roi_down_schedule(int hh, int ww, int patch, int n_up, const int *up_channels, int n_down, const int *down_channels,
                                      unsigned fused_mask, int form, int k, int *info, int *n_segs, int *segs, int const_cap, int *n_const,
                                      int *const_fills, int copy_cap, int *n_copy, int *copies)
{
    RoiPlan p;
    const bool args_ok = form >= ROI_DOWN_REGION && form <= ROI_DOWN_SHARE_FUSED_RECT && k >= 1 && info && n_segs && segs && n_const &&
                         const_fills && n_copy && copies && const_cap >= 0 && copy_cap >= 0;
    if (int rc = down_plan_for("tmat_roi_down_schedule", args_ok, hh, ww, patch, n_up, up_channels, n_down, down_channels, fused_mask, ROI_MAX_CLASSES, p))
        return rc;
    const RoiDownPlan &d = p.down;
    const RoiDownForm f = roi_down_form(p, (RoiDownForm)form);
    *n_const = *n_copy = 0;
    for (int l = 0; l < d.n_layers; l++) {
        RoiSegs sg;
        FillItems fi;
        std::vector<ShareItem> sh;
        roi_down_segs(p, f, l, k, sg);
        roi_down_const_items(p, f, l, k, fi);
        roi_down_copy_items(p, f, l, k, sh);
        n_segs[l] = sg.nseg;
        for (int i = 0; i < sg.nseg; i++) {
            const int o[6] = {sg.s[i].p0, sg.s[i].np, sg.s[i].y0, sg.s[i].x0, sg.s[i].rh, sg.s[i].rw};
            std::copy(o, o + 6, segs + ((size_t)l * ROI_MAX_SEGS + i) * 6);
        }
        if (*n_const + fi.n > const_cap || *n_copy + (int)sh.size() > copy_cap) { set_error("tmat_roi_down_schedule: cap too small"); return TMAT_E_ARG; }
        for (int i = 0; i < fi.n; i++, ++*n_const) {
            const int o[7] = {l, fi.it[i].p0, fi.it[i].np, fi.it[i].y0, fi.it[i].x0, fi.it[i].rh, fi.it[i].rw};
            std::copy(o, o + 7, const_fills + (size_t)*n_const * 7);
        }
        for (const ShareItem &c : sh) {
            const int o[8] = {l, c.p0, c.np, c.dir, c.y0, c.x0, c.rh, c.rw};
            std::copy(o, o + 8, copies + (size_t)(*n_copy)++ * 8);
        }
    }
    info[0] = f; info[1] = roi_down_stem_layer(p, f); info[2] = info[3] = 0;
    auto launch = [&](int l) { info[2] = std::max(info[2], n_segs[l]); info[3] += n_segs[l]; };
    if (d.fused_mask & 1u) launch(info[1]);
    for (int b = 0; b < d.n_down; b++)
        for (int kk = ((d.fused_mask >> b) & 1u) ? 4 : 0; kk < 6; kk++) launch(6 * b + kk);
    return TMAT_OK;
}
