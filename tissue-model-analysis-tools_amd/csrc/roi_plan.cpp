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
Iv align_to(Iv v, int al, int R) { return Iv{v.lo / al * al, std::min(R, (v.hi + al - 1) / al * al)}; }

// one class: rows[l] / cols[l] for every layer, from the interval of final outputs the blend reads on each axis
void walk_back(Iv orow, Iv ocol, int ws, int n_up, Iv *rows, Iv *cols)
{
    const int L = 3 * n_up + 1;
    int R = ws / 2;                                          // stored resolution of the final convolution
    // final_kernel: one thread = the 2 x 2 outputs above a stored pixel, one workgroup = 8 x 16 stored pixels, skipped or run as a whole
    rows[L - 1] = align_to(halve(orow), 8, R);
    cols[L - 1] = align_to(halve(ocol), 16, R);
    Iv need_r = dilate(rows[L - 1], 1, R), need_c = dilate(cols[L - 1], 1, R);      // of the last block's output
    for (int j = n_up - 1; j >= 0; j--) {
        const int Hl = R, Hs = j ? R / 2 : R;
        // second 3x3 (writes the block output and its activated copy): reads t1 one pixel around, the residual at (y >> up, x >> up)
        const Iv c2r = need_r, c2c = align_cols(need_c, Hl);
        rows[3 * j + 2] = c2r; cols[3 * j + 2] = c2c;
        const Iv t1r = dilate(c2r, 1, Hl), t1c = dilate(c2c, 1, Hl);
        const Iv rsr = j ? halve(c2r) : c2r, rsc = align_cols(j ? halve(c2c) : c2c, Hs);
        rows[3 * j + 1] = rsr; cols[3 * j + 1] = rsc;
        // first convolution.  Sub-pixel form (j > 0): stored pixel i makes the outputs 2 i and 2 i + 1 from the stored pixels i - 1 .. i + 1
        const Iv c1r = j ? halve(t1r) : t1r, c1c = align_cols(j ? halve(t1c) : t1c, Hs);
        rows[3 * j] = c1r; cols[3 * j] = c1c;
        // what the block reads of the previous block's output: the residual 1x1 its plain form, the first convolution its activated copy
        need_r = hull(rsr, dilate(c1r, 1, Hs));
        need_c = hull(rsc, dilate(c1c, 1, Hs));
        R = Hs;
    }
}

}  // namespace

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
        for (int l = 0; l < out.n_layers; l++) out.mac_planned[l] = out.mac_full[l];
        return true;
    }
    out.n_classes = (int)keys.size();
    for (int k = 0; k < out.n_classes; k++) out.class_base[k + 1] = out.class_base[k] + out.class_count[k];
    for (int k = 0; k < out.n_classes; k++) {
        Iv rows[ROI_MAX_LAYERS], cols[ROI_MAX_LAYERS];
        const bool empty = keys[k].r.hi <= keys[k].r.lo;
        if (!empty) walk_back(keys[k].r, keys[k].c, ws, n_up, rows, cols);
        for (int l = 0; l < out.n_layers; l++) {
            RoiRect q{0, 0, 0, 0};
            if (!empty) q = RoiRect{rows[l].lo, cols[l].lo, rows[l].hi - rows[l].lo, cols[l].hi - cols[l].lo};
            out.rect[l][k] = q;
            out.mac_planned[l] += mpp[l] * q.rh * q.rw * out.class_count[k];
        }
    }
    return true;
}

}  // namespace tmat

using namespace tmat;

extern "C" int tmat_roi_plan(int hh, int ww, int patch, int n_up, const int *channels, int max_classes, int tiles_cap, int *tiles_per_img,
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
            const RoiRect q = k < p.n_classes ? p.rect[l][k] : RoiRect{0, 0, 0, 0};
            int *o = rects + ((size_t)l * max_classes + k) * 4;
            o[0] = q.y0; o[1] = q.x0; o[2] = q.rh; o[3] = q.rw;
        }
        mac_planned[l] = p.mac_planned[l];
        mac_full[l] = p.mac_full[l];
    }
    return TMAT_OK;
}
