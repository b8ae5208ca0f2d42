// Tree overlay and barcode pictures (reference compute_branches.py:431-450, topology.py:67-144) as RGB8 rasters of our own
// specification (DESIGN.md "Tree overlay and barcode pictures"): the host twin of overlay_kernels.hip, the barcode raster, and the
// C-ABI entry that runs the rasteriser on the device.  Host twin and kernel share every formula through overlay.h.
#include "../../include/tmat.h"
#include "overlay.h"
#include "png.h"
#include "tmat_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace tmat {

bool canvas_of(int bh, int bw, int vis_width, Canvas &cv)
{
    if (bh < 1 || bw < 1 || vis_width < 1) return false;
    cv.vw = vis_width;
    cv.vh = (int)std::nearbyint((double)vis_width * (double)bh / (double)bw);       // round half to even
    if (cv.vh < 1) return false;
    const float r = (float)(0.75 * (200.0 / 72.0) * ((double)vis_width / 2000.0));   // matplotlib's 1.5 pt line at 200 dpi
    cv.rp = r + 0.5f;
    return true;
}

// background pixels -> canvas coordinates (float32), colour of the branch; segments with a non-finite coordinate are dropped
int prep_segments(const double *segs, const int32_t *seg_branch, int count, int bh, int bw, const Canvas &cv, std::vector<OverlaySeg> &out)
{
    auto map = [](double v, int dst, int src) {
        float f = (float)v;
        float a = f + 0.5f;
        float b = a * (float)dst;
        float c = b / (float)src;
        return c - 0.5f;
    };
    for (int i = 0; i < count; i++) {
        const double *p = segs + 4 * (size_t)i;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]))) continue;
        if (seg_branch[i] < 0) { set_error("render_tree: negative branch index"); return TMAT_E_ARG; }
        uint8_t rgb[3];
        tmat_branch_color(seg_branch[i], rgb);
        OverlaySeg s;
        s.x1 = map(p[0], cv.vw, bw); s.y1 = map(p[1], cv.vh, bh);
        s.x2 = map(p[2], cv.vw, bw); s.y2 = map(p[3], cv.vh, bh);
        s.r = (float)rgb[0]; s.g = (float)rgb[1]; s.b = (float)rgb[2]; s.pad = 0.0f;
        if (!(std::isfinite(s.x1) && std::isfinite(s.y1) && std::isfinite(s.x2) && std::isfinite(s.y2))) continue;
        out.push_back(s);
    }
    return TMAT_OK;
}

namespace {

static bool offsets_ok(const int32_t *off, int n)
{
    if (off[0] != 0) return false;
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}

static float bg_at(const void *bg, int dtype, size_t i) { return dtype == 0 ? (float)((const uint16_t *)bg)[i] : ((const float *)bg)[i]; }

}  // namespace

int morse_tree_item(const int32_t *verts, int nv, const int32_t *edges, int ne, int fh, int fw, int smooth, int min_len, int max_len, int remove_isolated,
                    const uint8_t *pruning, double scaling_factor, int64_t *count, double *total_px, double *avg_px, std::vector<double> &segs,
                    std::vector<int32_t> &branch, double *bars, int cap_b, int *n_bars)
{
    const int cap_s = std::max(nv, 1);       // a forest has fewer edges than vertices
    segs.resize((size_t)cap_s * 4); branch.resize(cap_s);
    int ns = 0;
    const int rc = tmat_morse_tree(verts, nv, edges, ne, fh, fw, smooth, min_len, max_len, remove_isolated, pruning, scaling_factor, count, total_px, avg_px,
                                   segs.data(), branch.data(), cap_s, bars, cap_b, &ns, n_bars);
    segs.resize((size_t)ns * 4); branch.resize(ns);
    return rc;
}

int overlay_pair_dev(const void *bg, int bg_dtype, int k, int bh, int bw, const Canvas &cv, const std::vector<double> *segs,
                     const std::vector<int32_t> *branch, const OverlayWs &ws, std::vector<OverlaySeg> &ss, std::vector<int> &off, uint8_t *rgb_host,
                     const char *who, hipStream_t s)
{
    const size_t cper = (size_t)cv.vh * cv.vw * 3;
    auto fail = [who](const char *what, int rc) { set_error(std::string(who) + ": " + what); return rc; };
    ss.clear();
    off.assign(k + 1, 0);
    for (int i = 0; i < k; i++) {
        if (int rc = prep_segments(segs[i].data(), branch[i].data(), (int)branch[i].size(), bh, bw, cv, ss)) return rc;
        off[i + 1] = (int)ss.size();
    }
    if (ss.size() > ws.seg_cap) return fail("segment workspace too small", TMAT_E_CAP);
    if ((!ss.empty() && hipMemcpyAsync(ws.dseg, ss.data(), ss.size() * sizeof(OverlaySeg), hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipMemcpyAsync(ws.doff, off.data(), (size_t)(k + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return fail("segment upload failed", TMAT_E_HIP);
    if (overlay_render_dev(bg, bg_dtype, ws.dmm, k, bh, bw, ws.dseg, ws.doff, cv.vh, cv.vw, cv.rp, ws.drgb, s)) return fail("overlay launch failed", TMAT_E_HIP);
    if (rgb_host && hipMemcpyAsync(rgb_host, ws.drgb, (size_t)k * cper, hipMemcpyDeviceToHost, s) != hipSuccess) return fail("overlay copy failed", TMAT_E_HIP);
    return TMAT_OK;
}

}  // namespace tmat

using namespace tmat;

extern "C" int tmat_host_render_tree(const void *background, int bg_dtype, int n, int bh, int bw, const double *segs, const int32_t *seg_branch,
                                     const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out)
{
    Canvas cv;
    if (!background || (bg_dtype != 0 && bg_dtype != 1) || n < 0 || !seg_offsets || !rgb_out || !canvas_of(bh, bw, vis_width, cv) || !offsets_ok(seg_offsets, n) ||
        (seg_offsets[n] && (!segs || !seg_branch))) {
        set_error("tmat_host_render_tree: bad argument");
        return TMAT_E_ARG;
    }
    const size_t per = (size_t)bh * bw, cper = (size_t)cv.vh * cv.vw;
    std::vector<float> C(cper * 3);
    std::vector<int> sx(cv.vw);
    for (int x = 0; x < cv.vw; x++) sx[x] = ovl_sample_index(x, bw, cv.vw);
    for (int img = 0; img < n; img++) {
        float mn = bg_at(background, bg_dtype, img * per), mx = mn;
        for (size_t i = 1; i < per; i++) { float v = bg_at(background, bg_dtype, img * per + i); mn = std::min(mn, v); mx = std::max(mx, v); }
        for (int y = 0; y < cv.vh; y++) {
            const int sy = ovl_sample_index(y, bh, cv.vh);
            for (int x = 0; x < cv.vw; x++) {
                const float g = ovl_grey(bg_at(background, bg_dtype, img * per + (size_t)sy * bw + sx[x]), mn, mx);
                float *c = &C[((size_t)y * cv.vw + x) * 3];
                c[0] = g; c[1] = g; c[2] = g;
            }
        }
        std::vector<OverlaySeg> ss;
        const int s0 = seg_offsets[img], cnt = seg_offsets[img + 1] - s0;
        int rc = prep_segments(segs + 4 * (size_t)s0, seg_branch + s0, cnt, bh, bw, cv, ss);
        if (rc) return rc;
        const float reach = cv.rp + 1.0f;
        for (const OverlaySeg &s : ss) {            // painter's order; pixels beyond the capsule's reach have coverage 0 and keep their value exactly
            const float lox = std::min(s.x1, s.x2) - reach, hix = std::max(s.x1, s.x2) + reach;
            const float loy = std::min(s.y1, s.y2) - reach, hiy = std::max(s.y1, s.y2) + reach;
            if (hix < 0.0f || hiy < 0.0f || lox > (float)(cv.vw - 1) || loy > (float)(cv.vh - 1)) continue;
            const int xa = (int)std::max(0.0f, std::floor(lox)), xb = (int)std::min((float)(cv.vw - 1), std::ceil(hix));
            const int ya = (int)std::max(0.0f, std::floor(loy)), yb = (int)std::min((float)(cv.vh - 1), std::ceil(hiy));
            for (int y = ya; y <= yb; y++)
                for (int x = xa; x <= xb; x++) {
                    const float a = ovl_coverage(s, (float)x, (float)y, cv.rp);
                    float *c = &C[((size_t)y * cv.vw + x) * 3];
                    c[0] = ovl_blend(c[0], s.r, a); c[1] = ovl_blend(c[1], s.g, a); c[2] = ovl_blend(c[2], s.b, a);
                }
        }
        uint8_t *o = rgb_out + (size_t)img * cper * 3;
        for (size_t i = 0; i < cper * 3; i++) o[i] = (uint8_t)std::floor(C[i] + 0.5f);
    }
    return TMAT_OK;
}

// ms (may be null): HIP-event times of the call's four phases on its stream -- upload, min-max, render kernels, copy back
// png_out (may be null): the overlays leave as PNG files (png.h) of at most cap_each bytes instead of as rasters; rgb_out is then not used
static int render_tree_impl(tmat_handle hd, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs, const int32_t *seg_branch,
                            const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out, float *ms, uint8_t *png_out = nullptr, size_t cap_each = 0,
                            size_t *png_sizes = nullptr)
{
    Ctx *c = (Ctx *)hd;
    if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.0f;
    Canvas cv;
    if (!c || !background || (bg_dtype != 0 && bg_dtype != 1) || n < 0 || !seg_offsets || !(png_out ? (void *)png_sizes : (void *)rgb_out) || !canvas_of(bh, bw, vis_width, cv) ||
        !offsets_ok(seg_offsets, n) || (seg_offsets[n] && (!segs || !seg_branch))) {
        set_error("tmat_render_tree: bad argument");
        return TMAT_E_ARG;
    }
    PngShape pg{};
    if (png_out) {
        if (!png_shape(cv.vh, cv.vw, 3, pg)) { set_error("tmat_render_tree_png: canvas too large for one PNG file"); return TMAT_E_ARG; }
        if (cap_each < pg.bound) { set_error("tmat_render_tree_png: cap_each is below tmat_png_bound"); return TMAT_E_CAP; }
    }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t per = (size_t)bh * bw, esz = bg_dtype == 0 ? 2 : 4, cper = (size_t)cv.vh * cv.vw * 3;
    // canvas-space segments of all images, with the offsets of what survived the non-finite filter
    std::vector<OverlaySeg> ss;
    std::vector<int> off(n + 1, 0);
    for (int img = 0; img < n; img++) {
        const int s0 = seg_offsets[img];
        int rc = prep_segments(segs + 4 * (size_t)s0, seg_branch + s0, seg_offsets[img + 1] - s0, bh, bw, cv, ss);
        if (rc) return rc;
        off[img + 1] = (int)ss.size();
    }
    const size_t nseg = ss.size();
    const int K = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)512 << 20) / cper));      // <= 512 MiB of canvases per launch
    uint8_t *dbg = (uint8_t *)ws_get(c, WS_TREE_BG, (size_t)n * per * esz);
    OverlaySeg *dseg = (OverlaySeg *)ws_get(c, WS_TREE_SEG, nseg * sizeof(OverlaySeg));
    float *dmm = (float *)ws_get(c, WS_TREE_MM, (size_t)n * 4 * sizeof(float) + (size_t)(n + 1) * sizeof(int));
    uint8_t *drgb = (uint8_t *)ws_get(c, WS_TREE_RGB, (size_t)K * cper);
    if (!dbg || !dseg || !dmm || !drgb) return TMAT_E_HIP;
    int *doff = (int *)(dmm + 4 * (size_t)n);
    hipStream_t s = c->stream;
    struct Events { hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); } } ev;
    DevScope mem(c->ws_pool, s);        // after ev: the events go when the stream has drained
    if (ms) for (hipEvent_t &e : ev.e) mem.check(hipEventCreate(&e), "hipEventCreate");
    auto mark = [&](int i) { if (ms && mem.ok) mem.check(hipEventRecord(ev.e[i], s), "hipEventRecord"); };
    auto span = [&](int a, int b, int slot) { float t = 0.0f; if (ms && hipEventElapsedTime(&t, ev.e[a], ev.e[b]) == hipSuccess) ms[slot] += t; };
    mark(0);
    mem.h2d(dbg, background, (size_t)n * per * esz);
    if (nseg) mem.h2d(dseg, mem.keep(std::move(ss)), nseg * sizeof(OverlaySeg));
    mem.h2d(doff, mem.keep(std::move(off)), (size_t)(n + 1) * sizeof(int));
    mark(1);
    if (!mem.ok) return TMAT_E_HIP;
    if (overlay_minmax_dev(dbg, bg_dtype, n, bh, bw, dmm, s)) { set_error("tmat_render_tree: min-max launch failed"); return TMAT_E_HIP; }
    mark(2);
    if (ms) {
        if (mem.finish()) return TMAT_E_HIP;
        span(0, 1, 0); span(1, 2, 1);
    }
    for (int i0 = 0; i0 < n; i0 += K) {
        const int k = std::min(K, n - i0);
        mark(0);
        const int r = overlay_render_dev(dbg + (size_t)i0 * per * esz, bg_dtype, dmm + 2 * (size_t)i0, k, bh, bw, dseg, doff + i0, cv.vh, cv.vw, cv.rp, drgb, s);
        if (r == -1) { set_error("tmat_render_tree: canvas too large for one launch"); return TMAT_E_ARG; }
        if (r) { set_error("tmat_render_tree: kernel launch failed"); return TMAT_E_HIP; }
        mark(1);
        if (png_out) {      // the encoder follows on the same stream; only file bytes cross to the host
            if (int rc = png_encode_ctx(c, drgb, false, k, pg, png_out + (size_t)i0 * cap_each, cap_each, png_sizes + i0, nullptr)) return rc;
        } else {
            mem.d2h(rgb_out + (size_t)i0 * cper, drgb, (size_t)k * cper);
        }
        mark(2);
        if (mem.finish()) return TMAT_E_HIP;
        span(0, 1, 2); span(1, 2, 3);
    }
    return TMAT_OK;
}

extern "C" int tmat_render_tree(tmat_handle hd, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs, const int32_t *seg_branch,
                                const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out)
{
    return render_tree_impl(hd, background, bg_dtype, n, bh, bw, segs, seg_branch, seg_offsets, vis_width, rgb_out, nullptr);
}

extern "C" int tmat_render_tree_timed(tmat_handle hd, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs,
                                      const int32_t *seg_branch, const int32_t *seg_offsets, int vis_width, uint8_t *rgb_out, float *ms4)
{
    if (!ms4) { set_error("tmat_render_tree_timed: bad argument"); return TMAT_E_ARG; }
    return render_tree_impl(hd, background, bg_dtype, n, bh, bw, segs, seg_branch, seg_offsets, vis_width, rgb_out, ms4);
}

extern "C" int tmat_render_tree_png(tmat_handle hd, const void *background, int bg_dtype, int n, int bh, int bw, const double *segs,
                                    const int32_t *seg_branch, const int32_t *seg_offsets, int vis_width, uint8_t *out, size_t cap_each, size_t *sizes)
{
    if (!out) { set_error("tmat_render_tree_png: bad argument"); return TMAT_E_ARG; }
    return render_tree_impl(hd, background, bg_dtype, n, bh, bw, segs, seg_branch, seg_offsets, vis_width, nullptr, nullptr, out, cap_each, sizes);
}

// plot_colored_barcode (topology.py:67-107) without axes or text.  What needs a sequential host -- the stable sort by birth, the edge
// rounding, the branch colours -- ends in a table of rectangles; the host twin and barcode_kernel (overlay_kernels.hip) fill the same table.
namespace tmat {

int barcode_side(int vis_width) { return (int)std::nearbyint((double)vis_width * 0.9); }

void barcode_rects(const double *bars, int n, int S, std::vector<BarRect> &out)
{
    if (n < 1) return;
    double lo = bars[0], hi = bars[1];
    for (int i = 0; i < n; i++) { lo = std::min(lo, bars[2 * i]); hi = std::max(hi, bars[2 * i + 1]); }
    const double span = hi - lo;
    if (!(span > 0.0) || !std::isfinite(span)) return;
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bars[2 * a] > bars[2 * b]; });     // birth, descending
    const double pitch = (double)S / (double)n;
    auto edge = [&](double v) {
        double e = std::floor((v - lo) / span * (double)S + 0.5);
        return (int)std::min((double)S, std::max(0.0, e));
    };
    for (int k = 0; k < n; k++) {
        const int bi = order[k];
        uint8_t col[3];
        tmat_branch_color(bi, col);
        BarRect r;
        r.xa = edge(bars[2 * bi]); r.xb = edge(bars[2 * bi + 1]);
        r.ya = (int)std::floor(((double)k + 0.1) * pitch + 0.5); r.yb = (int)std::floor(((double)k + 0.9) * pitch + 0.5);
        r.rgb = (uint32_t)col[0] | ((uint32_t)col[1] << 8) | ((uint32_t)col[2] << 16);
        out.push_back(r);
    }
}

void barcode_fill_host(const BarRect *rects, int n, int S, uint8_t *rgb)
{
    std::memset(rgb, 255, (size_t)S * S * 3);
    for (int k = 0; k < n; k++) {
        const BarRect &r = rects[k];
        const uint8_t col[3] = {(uint8_t)(r.rgb & 255u), (uint8_t)((r.rgb >> 8) & 255u), (uint8_t)((r.rgb >> 16) & 255u)};
        for (int y = r.ya; y < r.yb; y++) {        // bar 0 is the lowest row of the picture, as on matplotlib's upward y axis
            uint8_t *row = rgb + (size_t)(S - 1 - y) * S * 3;
            for (int x = r.xa; x < r.xb; x++) { row[3 * x] = col[0]; row[3 * x + 1] = col[1]; row[3 * x + 2] = col[2]; }
        }
    }
}

}  // namespace tmat

extern "C" int tmat_host_render_barcode(const double *bars, int n, int vis_width, uint8_t *rgb_out)
{
    if (n < 0 || (n && !bars) || vis_width < 1 || !rgb_out) { set_error("tmat_host_render_barcode: bad argument"); return TMAT_E_ARG; }
    const int S = barcode_side(vis_width);
    if (S < 1) { set_error("tmat_host_render_barcode: empty canvas"); return TMAT_E_ARG; }
    std::vector<BarRect> rects;
    barcode_rects(bars, n, S, rects);
    barcode_fill_host(rects.data(), (int)rects.size(), S, rgb_out);
    return TMAT_OK;
}

// test entry of the shared helper: the rectangles of one picture, (xa, xb, ya, yb, rgb) as five int32 each; *n_rects may be 0 (nothing drawn)
extern "C" int tmat_host_barcode_rects(const double *bars, int n, int vis_width, int32_t *rects_out, int cap, int *n_rects)
{
    if (n < 0 || (n && !bars) || vis_width < 1 || cap < 0 || (cap && !rects_out) || !n_rects) { set_error("tmat_host_barcode_rects: bad argument"); return TMAT_E_ARG; }
    const int S = barcode_side(vis_width);
    if (S < 1) { set_error("tmat_host_barcode_rects: empty canvas"); return TMAT_E_ARG; }
    std::vector<BarRect> rects;
    barcode_rects(bars, n, S, rects);
    *n_rects = (int)rects.size();
    if ((int)rects.size() > cap) { set_error("tmat_host_barcode_rects: cap is below the number of rectangles"); return TMAT_E_CAP; }
    for (size_t k = 0; k < rects.size(); k++) {
        int32_t *o = rects_out + 5 * k;
        o[0] = rects[k].xa; o[1] = rects[k].xb; o[2] = rects[k].ya; o[3] = rects[k].yb; o[4] = (int32_t)rects[k].rgb;
    }
    return TMAT_OK;
}

// png_out (may be null): the canvases leave as PNG files (png.h) instead of as rasters; rgb_out is then not used
static int render_barcode_impl(tmat_handle hd, const char *who, const double *bars, const int32_t *bar_offsets, int n_pics, int vis_width, uint8_t *rgb_out,
                               uint8_t *png_out, size_t cap_each, size_t *png_sizes)
{
    Ctx *c = (Ctx *)hd;
    const int S = vis_width >= 1 ? barcode_side(vis_width) : 0;
    if (!c || n_pics < 0 || !bar_offsets || vis_width < 1 || S < 1 || !(png_out ? (void *)png_sizes : (void *)rgb_out) || !offsets_ok(bar_offsets, n_pics) ||
        (bar_offsets[n_pics] && !bars)) {
        set_error(std::string(who) + ": bad argument");
        return TMAT_E_ARG;
    }
    PngShape pg{};
    if (png_out) {
        if (!png_shape(S, S, 3, pg)) { set_error(std::string(who) + ": canvas too large for one PNG file"); return TMAT_E_ARG; }
        if (cap_each < pg.bound) { set_error(std::string(who) + ": cap_each is below tmat_png_bound"); return TMAT_E_CAP; }
    }
    if (n_pics == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    std::vector<BarRect> rects;
    std::vector<int> off(n_pics + 1, 0);
    for (int p = 0; p < n_pics; p++) {
        barcode_rects(bars + 2 * (size_t)bar_offsets[p], bar_offsets[p + 1] - bar_offsets[p], S, rects);
        off[p + 1] = (int)rects.size();
    }
    const size_t cper = (size_t)S * S * 3, nrect = rects.size();
    const int K = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_pics, ((size_t)512 << 20) / cper));      // <= 512 MiB of canvases per launch
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    BarRect *drect = mem.pooled<BarRect>(nrect);
    int *doff = mem.pooled<int>((size_t)n_pics + 1);
    uint8_t *drgb = mem.pooled<uint8_t>((size_t)K * cper);
    if (nrect) mem.h2d(drect, mem.keep(std::move(rects)), nrect * sizeof(BarRect));
    mem.h2d(doff, mem.keep(std::move(off)), ((size_t)n_pics + 1) * sizeof(int));
    if (!mem.ok) return TMAT_E_HIP;
    for (int i0 = 0; i0 < n_pics; i0 += K) {
        const int k = std::min(K, n_pics - i0);
        const int r = barcode_render_dev(drect, doff + i0, k, S, drgb, s);
        if (r) { set_error(std::string(who) + (r == -1 ? ": canvas too large for one launch" : ": kernel launch failed")); return r == -1 ? TMAT_E_ARG : TMAT_E_HIP; }
        if (png_out) {      // the encoder follows on the same stream; only file bytes cross to the host
            if (int rc = png_encode_ctx(c, drgb, false, k, pg, png_out + (size_t)i0 * cap_each, cap_each, png_sizes + i0, nullptr)) return rc;
        } else {
            mem.d2h(rgb_out + (size_t)i0 * cper, drgb, (size_t)k * cper);
        }
        if (mem.finish()) return TMAT_E_HIP;
    }
    return TMAT_OK;
}

extern "C" int tmat_render_barcode(tmat_handle hd, const double *bars, const int32_t *bar_offsets, int n_pics, int vis_width, uint8_t *rgb_out)
{
    return render_barcode_impl(hd, "tmat_render_barcode", bars, bar_offsets, n_pics, vis_width, rgb_out, nullptr, 0, nullptr);
}

extern "C" int tmat_render_barcode_png(tmat_handle hd, const double *bars, const int32_t *bar_offsets, int n_pics, int vis_width, uint8_t *out, size_t cap_each,
                                       size_t *sizes)
{
    if (!out) { set_error("tmat_render_barcode_png: bad argument"); return TMAT_E_ARG; }
    return render_barcode_impl(hd, "tmat_render_barcode_png", bars, bar_offsets, n_pics, vis_width, nullptr, out, cap_each, sizes);
}

