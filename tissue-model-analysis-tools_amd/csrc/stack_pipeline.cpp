// Driver of the Z-stack (Sato) branch of analyze_img (reference scripts/compute_branches.py:224-306 and the common tail
// :391-457) behind include/tmat.h: tmat_gaussian_f32, tmat_sato_batch, tmat_stack_prepare, tmat_vessel_field,
// tmat_analyze_stack.  The pixel stages are the kernels of sato_kernels.hip plus the medial axis (thin_kernels.hip), the
// mask filter (morph_kernels.hip) and the DMT front end (dmt_kernels.hip) of the 2-D path; the host contributes the gaussian
// tables (gauss_tables.cpp), the medial axis' tie-break permutation and the sequential graph sweeps (dmt.cpp, morse.cpp).
#include "../../include/tmat.h"
#include "tmat_ctx.h"
#include "postproc.h"
#include "morph.h"
#include "sato.h"
#include "wellmask.h"
#include "overlay.h"
#include "host_par.h"

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <thread>

namespace tmat {

int medial_thin_batch_dev(Ctx *c, const uint8_t *mask_dev, const double *dist_dev, int k, int hh, int ww, uint8_t *skel_dev, hipStream_t s);
void zoom_axis_table(int n_in, int n_out, std::vector<int> &i0, std::vector<int> &i1, std::vector<double> &a0, std::vector<double> &a1);

namespace {

// device copy of a gaussian table, made on first use (synchronous copy: a few hundred doubles)
const double *table_dev(Ctx *c, const GaussTable &t)
{
    auto it = c->gauss_dev.find(&t);
    if (it != c->gauss_dev.end()) return it->second;
    double *d = nullptr;
    if (!hip_ok(hipMalloc((void **)&d, t.w.size() * sizeof(double)), "hipMalloc")) return nullptr;
    if (!hip_ok(hipMemcpy(d, t.w.data(), t.w.size() * sizeof(double), hipMemcpyHostToDevice), "H2D")) { hipFree(d); return nullptr; }
    c->gauss_dev[&t] = d;
    return d;
}

struct Pass { double sigma; int order; int L, inner; size_t outer; };

// one 1-D pass of ndi.gaussian_filter on f32 data
bool gauss_pass_f32(Ctx *c, const float *in, float *out, const Pass &p, double truncate, int mode, hipStream_t s)
{
    const GaussTable &t = gauss_table(c, p.sigma, p.order, gauss_radius(p.sigma, truncate));
    const double *w = table_dev(c, t);
    if (!w) return false;
    launch_corr1d_f32(in, out, p.outer, p.L, p.inner, w, t.r, t.sym, mode, s);
    return true;
}

// ndi.gaussian_filter(x, sigma, order=(o0, o1), mode, truncate) on n images (h, w): axis 0 then axis 1, f32 after each pass
bool gauss2d_f32(Ctx *c, const float *in, float *tmp, float *out, int n, int h, int w, double sigma, int o0, int o1, double truncate, int mode,
                 hipStream_t s)
{
    return gauss_pass_f32(c, in, tmp, Pass{sigma, o0, h, w, (size_t)n}, truncate, mode, s) &&
           gauss_pass_f32(c, tmp, out, Pass{sigma, o1, w, 1, (size_t)n * h}, truncate, mode, s);
}

// skimage.filters.sato(im, sigmas, black_ridges=False) on n images; x = the prepared input (1 - im or -im), best = result.
// bufs: 7 arrays of n h w floats
bool sato_dev(Ctx *c, const float *x, int n, int h, int w, const double *sigmas, int nsig, int form, float *const bufs[7], float *best, hipStream_t s)
{
    const size_t total = (size_t)n * h * w;
    float *T = bufs[0], *G0 = bufs[1], *G1 = bufs[2], *H0 = bufs[3], *H1 = bufs[4], *H2 = bufs[5], *T2 = bufs[6];
    if (nsig == 0) return hip_ok(hipMemsetAsync(best, 0, total * sizeof(float), s), "memset");
    for (int k = 0; k < nsig; k++) {
        const double sg = sigmas[k];
        const float s2 = (float)(sg * sg);
        if (form == TMAT_SATO_GAUSSIAN_DERIVATIVES) {
            // hessian_matrix(use_gaussian_derivatives=True): sigma / sqrt(2) twice, truncate 8 (100 when sigma <= 1), 'reflect'
            const double sq1_2 = 1.0 / std::sqrt(2.0);
            const double ss = sq1_2 * sg, tr = sg > 1.0 ? 8.0 : 100.0;
            if (!gauss2d_f32(c, x, T, G0, n, h, w, ss, 1, 0, tr, EXT_REFLECT, s) || !gauss2d_f32(c, x, T, G1, n, h, w, ss, 0, 1, tr, EXT_REFLECT, s) ||
                !gauss2d_f32(c, G0, T, H0, n, h, w, ss, 1, 0, tr, EXT_REFLECT, s) || !gauss2d_f32(c, G0, T, H1, n, h, w, ss, 0, 1, tr, EXT_REFLECT, s) ||
                !gauss2d_f32(c, G1, T, H2, n, h, w, ss, 0, 1, tr, EXT_REFLECT, s)) return false;
            launch_eig(1, H0, H1, H2, s2, total, best, k == 0, s);
        } else {
            // hessian_matrix of scikit-image <= 0.19: gaussian (truncate 4, 'reflect'), np.gradient twice, elements scaled by sigma^2
            if (!gauss2d_f32(c, x, T, G0, n, h, w, sg, 0, 0, 4.0, EXT_REFLECT, s)) return false;
            launch_gradient(G0, G1, (size_t)n, h, w, s);              // d/dr
            launch_gradient(G0, H0, (size_t)n * h, w, 1, s);          // d/dc
            launch_gradient(G1, H1, (size_t)n, h, w, s);              // Hrr
            launch_gradient(H0, H2, (size_t)n, h, w, s);              // Hrc = d/dr of d/dc
            launch_gradient(H0, T2, (size_t)n * h, w, 1, s);          // Hcc
            launch_eig(0, H1, H2, T2, s2, total, best, k == 0, s);
        }
    }
    return hipGetLastError() == hipSuccess;
}

const double SATO_SIGMAS[10] = {1, 2, 3, 4, 5, 7, 9, 11, 13, 15};       // compute_branches.py:262

}  // namespace

// n volumes (n, Z, h, w) f32 on the device -> n fields (n, h, w) f32 on the device, one launch set for all of them; stage copies go to
// the host arrays of `st` that are non-null (each with a leading n).  Every per-image quantity -- labels, moment tables, convergence
// flags, borders of the neighbourhood stages -- is indexed by the volume; the Sato chain sees n (Z - 1) independent images.
int vessel_field_dev(Ctx *c, const float *vol, int n, int Z, int h, int w, int form, float *field, const tmat_vessel_stages *st, hipStream_t s)
{
    if (n < 1) { set_error("vessel field: no volume"); return TMAT_E_ARG; }
    if (Z < 2) { set_error("vessel field: a Z stack needs at least 2 slices"); return TMAT_E_ARG; }
    if (!thin_dev_supported(h, w)) { set_error("vessel field: image too large for the device thinning kernel"); return TMAT_E_ARG; }
    const int D = Z - 1;
    const size_t px1 = (size_t)h * w, npx = (size_t)n * px1, nv = (size_t)D * npx;     // npx, nv: over the n volumes
    DevScope A(c->ws_pool, s);
    float *x = A.pooled<float>(nv), *vess = A.pooled<float>(nv), *bufs[7];
    for (float *&b : bufs) b = A.pooled<float>(nv);
    float *vessels = A.pooled<float>(npx), *vcur = A.pooled<float>(npx), *vblur = A.pooled<float>(npx), *vtmp = A.pooled<float>(npx);
    CannyWs cw{};
    cw.sm = A.pooled<double>(npx); cw.t0 = A.pooled<double>(npx); cw.is_ = A.pooled<double>(npx); cw.js = A.pooled<double>(npx); cw.mag = A.pooled<double>(npx);
    cw.low = A.pooled<uint8_t>(npx); cw.high = A.pooled<uint8_t>(npx); cw.L = A.pooled<int>(npx); cw.flag = A.pooled<int>(npx);
    double *tabs = A.pooled<double>(6);
    uint8_t *edges = A.pooled<uint8_t>(npx), *skel = A.pooled<uint8_t>(npx), *m0 = A.pooled<uint8_t>(npx), *m1 = A.pooled<uint8_t>(npx), *filt = A.pooled<uint8_t>(npx);
    double *dist = A.pooled<double>(npx);
    int *edt_g = A.pooled<int>(npx), *anyz = A.pooled<int>(std::max(n, 4));
    unsigned long long *mom = A.pooled<unsigned long long>(npx * 6);
    int *offs = A.pooled<int>(2 * (13 + 9));
    void *mws = A.pooled_bytes(morph_workspace_bytes(n, h, w));
    if (!A.ok) return TMAT_E_HIP;
    {
        std::vector<int> o;
        for (int dy = -2; dy <= 2; dy++) for (int dx = -2; dx <= 2; dx++) if (dy * dy + dx * dx <= 4) { o.push_back(dy); o.push_back(dx); }       // disk(2): 13
        for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) { o.push_back(dy); o.push_back(dx); }                                   // square(3): 9
        A.h2d(tabs, A.keep(std::vector<double>{-1.0, 0.0, 1.0, 1.0, 2.0, 1.0}), 6 * sizeof(double));
        A.h2d(offs, A.keep(std::move(o)), 2 * 22 * sizeof(int));
        if (!A.ok) return TMAT_E_HIP;
    }
    cw.w_diff = tabs; cw.w_smooth = tabs + 3;
    const bool deriv = form == TMAT_SATO_GAUSSIAN_DERIVATIVES;

    // z4: Sato of max(slice z, slice z + 1), all D pairs in one launch per pass
    launch_pairmax(vol, n, D, px1, deriv ? 1 : 0, x, s);
    if (!sato_dev(c, x, n * D, h, w, SATO_SIGMAS, 10, form, bufs, vess, s)) { set_error("vessel field: Sato stage failed"); return TMAT_E_HIP; }
    if (st) A.d2h(st->vess, vess, nv * 4);
    // z5: unsharp_mask(volume, radius 2, amount 2): 3-D gaussian ('reflect', truncate 4) over Z, rows, columns
    float *sharp = x;                                                        // x is free from here on
    if (!gauss_pass_f32(c, vess, bufs[0], Pass{2.0, 0, D, (int)px1, (size_t)n}, 4.0, EXT_REFLECT, s) ||
        !gauss_pass_f32(c, bufs[0], bufs[1], Pass{2.0, 0, h, w, (size_t)n * D}, 4.0, EXT_REFLECT, s) ||
        !gauss_pass_f32(c, bufs[1], bufs[0], Pass{2.0, 0, w, 1, (size_t)n * D * h}, 4.0, EXT_REFLECT, s)) return TMAT_E_HIP;
    launch_unsharp(vess, bufs[0], 2.0f, nv, sharp, s);
    launch_zmax(sharp, n, D, px1, vessels, s);
    if (st) { A.d2h(st->sharp, sharp, nv * 4); A.d2h(st->vessels, vessels, npx * 4); }
    // z6: canny
    if (canny0_dev(vessels, n, h, w, cw, edges, s)) { set_error("vessel field: canny stage failed"); return TMAT_E_HIP; }
    if (st) A.d2h(st->edges, edges, npx);
    // z7: medial axis of the edges; keep skeleton components with eccentricity * equivalent diameter > 3.5
    launch_edt(edges, n, h, w, edt_g, nullptr, anyz, dist, s);
    { int rc = medial_thin_batch_dev(c, edges, dist, n, h, w, skel, s); if (rc) return rc; }
    if (ecc_diam_select_dev(skel, n, h, w, 3.5, cw.L, mom, m0, nullptr, s)) return TMAT_E_HIP;
    if (st) { A.d2h(st->skel, skel, npx); A.d2h(st->mask_sel, m0, npx); }
    // z8: three masked blurs of the projection
    if (!A.check(hipMemcpyAsync(vcur, vessels, npx * 4, hipMemcpyDeviceToDevice, s), "D2D")) return TMAT_E_HIP;
    for (int it = 0; it < 3; it++) {
        if (!gauss2d_f32(c, vcur, vtmp, vblur, n, h, w, 1.0, 0, 0, 4.0, EXT_NEAREST, s)) return TMAT_E_HIP;
        launch_where(m0, vblur, vcur, npx, vtmp, s);
        std::swap(vcur, vtmp);
    }
    //     ten region-growing rounds, mask &= ~edges, closing with disk(2)
    uint8_t *ma = m0, *mb = m1;
    for (int it = 0; it < 10; it++) { launch_grow(ma, vcur, n, h, w, mb, s); std::swap(ma, mb); }
    if (st) A.d2h(st->grown, ma, npx);
    launch_andnot(ma, edges, npx, mb, s);
    launch_morph(mb, n, h, w, offs, 13, 0, ma, s);
    launch_morph(ma, n, h, w, offs, 13, 1, mb, s);
    if (st) A.d2h(st->closed, mb, npx);
    // z9: filter_branch_seg_mask(mask, None, False), dilation with square(3), mask the sharpened projection, gaussian
    if (filter_mask_dev(nullptr, mb, n, h, w, 0, 0, mws, filt, nullptr, s)) return TMAT_E_HIP;
    int *conv = A.host<int>(n);
    A.d2h(conv, morph_done_flags(mws, n, h, w), n * sizeof(int));
    launch_morph(filt, n, h, w, offs + 26, 9, 0, ma, s);
    launch_where(ma, vessels, nullptr, npx, vtmp, s);
    if (!gauss2d_f32(c, vtmp, vblur, field, n, h, w, 1.0, 0, 0, 4.0, EXT_NEAREST, s)) return TMAT_E_HIP;
    if (st) A.d2h(st->filt, filt, npx);
    if (A.finish()) return TMAT_E_HIP;
    if (hipGetLastError() != hipSuccess) { set_error("vessel field: kernel launch failed"); return TMAT_E_HIP; }
    for (int i = 0; i < n; i++) if (!conv[i]) { set_error("vessel field: thinning did not converge"); return TMAT_E_HIP; }
    return TMAT_OK;
}

// stack (Z, H, W) u16 on the device (overwritten by its per-slice gaussian) -> vol (Z, oh, ow) f32 on the device
// skimage.transform.resize(stack, (Z, oh, ow), order=1, preserve_range=True, anti_aliasing=True) of an integer stack (scikit-image
// >= 0.19: ndi.gaussian_filter(sigma (factor - 1) / 2, 'mirror') + ndi.zoom(order 1, grid_mode) on the 3-D array, the Z axis with sigma 0
// and zoom 1), clipped to the stack's range: the float64 values in `zoomed` (device, Z oh ow); with `vol` also rescale_intensity(0..1) over
// the whole stack as float32.  n stacks (n, Z, H, W) go through one launch set; the clip range and the rescale are per stack
int stack_resize_aa_dev(Ctx *c, const uint16_t *stack, int n, int Z, int H, int W, int oh, int ow, double *zoomed, float *vol, hipStream_t s)
{
    const size_t nin = (size_t)n * Z * H * W, NZ = (size_t)n * Z;
    DevScope A(c->ws_pool, s);
    double *fa = A.pooled<double>(nin), *fb = A.pooled<double>(nin), *lohi = A.pooled<double>(4 * (size_t)n);
    unsigned long long *mm = A.pooled<unsigned long long>(2 * (size_t)n);
    std::vector<int> r0, r1, c0, c1;
    std::vector<double> wr0, wr1, wc0, wc1;
    zoom_axis_table(H, oh, r0, r1, wr0, wr1);
    zoom_axis_table(W, ow, c0, c1, wc0, wc1);
    int *dr0 = A.pooled<int>(oh), *dr1 = A.pooled<int>(oh), *dc0 = A.pooled<int>(ow), *dc1 = A.pooled<int>(ow);
    double *dwr0 = A.pooled<double>(oh), *dwr1 = A.pooled<double>(oh), *dwc0 = A.pooled<double>(ow), *dwc1 = A.pooled<double>(ow);
    auto up = [&A](auto *dst, auto &table, int count) { A.h2d(dst, A.keep(std::move(table)), count * sizeof(*dst)); };     // the scope keeps the tables
    up(dr0, r0, oh); up(dr1, r1, oh); up(dc0, c0, ow); up(dc1, c1, ow);
    up(dwr0, wr0, oh); up(dwr1, wr1, oh); up(dwc0, wc0, ow); up(dwc1, wc1, ow);
    if (!A.ok) return TMAT_E_HIP;
    // anti-aliasing gaussian over rows and columns ('mirror', sigma (factor - 1) / 2), zoom, clip to the stack's range
    const double f0 = (double)H / (double)oh, f1 = (double)W / (double)ow;
    const double s0 = std::max(0.0, (f0 - 1) / 2), s1 = std::max(0.0, (f1 - 1) / 2);
    const double *cur = nullptr;
    if (s0 > 1e-15) {          // scipy skips an axis whose sigma is <= 1e-15
        const GaussTable &t = gauss_table(c, s0, 0, gauss_radius(s0, 4.0));
        const double *wd = table_dev(c, t);
        if (!wd) return TMAT_E_HIP;
        launch_corr1d_u16_f64(stack, fa, NZ, H, W, wd, t.r, t.sym, EXT_MIRROR, s);
        cur = fa;
    }
    if (s1 > 1e-15) {
        const GaussTable &t = gauss_table(c, s1, 0, gauss_radius(s1, 4.0));
        const double *wd = table_dev(c, t);
        if (!wd) return TMAT_E_HIP;
        if (cur) launch_corr1d_f64(cur, fb, NZ * H, W, 1, wd, t.r, t.sym, EXT_MIRROR, s);
        else launch_corr1d_u16_f64(stack, fb, NZ * H, W, 1, wd, t.r, t.sym, EXT_MIRROR, s);
        cur = fb;
    }
    if (!cur) {               // no smoothing at all (an image at most as wide as the target): the zoom reads the stack as f64
        double *w_id = lohi;   // borrowed for a moment: a 1-tap identity kernel
        if (!A.h2d(w_id, A.keep(std::vector<double>{1.0}), 8)) return TMAT_E_HIP;
        launch_corr1d_u16_f64(stack, fa, NZ * H, W, 1, w_id, 0, 1, EXT_MIRROR, s);
        cur = fa;
    }
    if (stack_zoom_rescale_dev(cur, stack, n, Z, H, W, oh, ow, dr0, dr1, dwr0, dwr1, dc0, dc1, dwc0, dwc1, zoomed, mm, lohi, vol, s)) {
        set_error("stack resize: kernel launch failed");
        return TMAT_E_HIP;
    }
    return A.finish();
}

// n stacks (n, Z, H, W) u16 on the device (overwritten) -> vol (n, Z, oh, ow) f32 on the device
int stack_prepare_dev(Ctx *c, uint16_t *stack, int n, int Z, int H, int W, int oh, int ow, float *vol, hipStream_t s)
{
    const size_t NZ = (size_t)n * Z, nin = NZ * H * W, nout = NZ * oh * ow;
    DevScope A(c->ws_pool, s);
    double *fa = A.pooled<double>(nin), *zoomed = A.pooled<double>(nout);
    if (!A.ok) return TMAT_E_HIP;
    // z1: gaussian(slice, sigma 1, 'nearest') in f64, written back into the integer stack (C truncation)
    const GaussTable &g1 = gauss_table(c, 1.0, 0, gauss_radius(1.0, 4.0));
    const double *w1 = table_dev(c, g1);
    if (!w1) return TMAT_E_HIP;
    launch_corr1d_u16_f64(stack, fa, NZ, H, W, w1, g1.r, g1.sym, EXT_NEAREST, s);
    launch_corr1d_f64_u16(fa, stack, NZ * H, W, 1, w1, g1.r, g1.sym, EXT_NEAREST, s);
    // z2 + z3: anti-aliased resize, rescale to 0..1 over each whole stack
    return stack_resize_aa_dev(c, stack, n, Z, H, W, oh, ow, zoomed, vol, s);
}

// well_mask_generation.py:153-155: the shape generate_well_mask searches on, round(shape * min(1, 200 / max(shape))) half to even
void well_small_shape(int h, int w, int *sh, int *sw)
{
    const double ratio = std::min(1.0, 200.0 / (double)std::max(h, w));
    *sh = (int)std::nearbyint((double)h * ratio);
    *sw = (int)std::nearbyint((double)w * ratio);
}

// auto_threshold_well (reference :236-277) of n images (n, H, W) in device memory, f64 (img64) or f32 (img32, n = 1 only; overwritten)
// -> thresholded, eroded masks `out` (n, H, W) u8 on the device.  img64 is overwritten by its gaussian
int well_threshold_dev(Ctx *c, double *img64, float *img32, int n, int H, int W, uint8_t *out, hipStream_t s)
{
    const size_t px = (size_t)H * W, tot = (size_t)n * px;
    DevScope A(c->ws_pool, s);
    uint8_t *u8 = A.pooled<uint8_t>(tot), *th = A.pooled<uint8_t>(tot);
    unsigned *hist = A.pooled<unsigned>((size_t)n * 5 * 256);
    int *decision = A.pooled<int>(2 * (size_t)n), *offs = A.pooled<int>(2 * 81);
    std::vector<int> o;
    for (int dy = -5; dy <= 5; dy++) for (int dx = -5; dx <= 5; dx++) if (dy * dy + dx * dx <= 25) { o.push_back(dy); o.push_back(dx); }         // disk(5): 81
    const int k = (int)o.size() / 2;
    A.h2d(offs, A.keep(std::move(o)), sizeof(int) * 2 * k);
    // gaussian(image, sigma=1): ndi.gaussian_filter, mode 'nearest', truncate 4, the image's float type after each axis
    if (img64) {
        double *db = A.pooled<double>(tot), *dmm = A.pooled<double>(2 * (size_t)n);
        if (!A.ok) return TMAT_E_HIP;
        const GaussTable &gt = gauss_table(c, 1.0, 0, gauss_radius(1.0, 4.0));
        const double *w = table_dev(c, gt);
        if (!w) return TMAT_E_HIP;
        launch_corr1d_f64(img64, db, (size_t)n, H, W, w, gt.r, gt.sym, EXT_NEAREST, s);
        launch_corr1d_f64(db, img64, (size_t)n * H, W, 1, w, gt.r, gt.sym, EXT_NEAREST, s);
        launch_wm_rescale_u8_f64(img64, n, px, dmm, u8, s);
    } else {
        if (n != 1) { set_error("well threshold: float32 images go one at a time"); return TMAT_E_ARG; }
        float *b = A.pooled<float>(px), *mm = A.pooled<float>(2);
        if (!A.ok) return TMAT_E_HIP;
        if (!gauss_pass_f32(c, img32, b, Pass{1.0, 0, H, W, 1}, 4.0, EXT_NEAREST, s) || !gauss_pass_f32(c, b, img32, Pass{1.0, 0, W, 1, (size_t)H}, 4.0, EXT_NEAREST, s))
            return TMAT_E_HIP;
        launch_minmax_f32(img32, 1, px, mm, mm + 1, s);
        launch_wm_rescale_u8(img32, px, mm, mm + 1, u8, s);
    }
    launch_wm_hist(u8, n, H, W, hist, s);
    launch_wm_decide(hist, n, H, W, decision, s);
    launch_wm_threshold(u8, n, px, decision, th, s);
    launch_wm_erode(th, n, H, W, offs, k, out, s);
    A.check(hipGetLastError(), "tmat_well_threshold: kernel launch");
    return A.finish();          // the scope's blocks go back to the pool: nothing may be in flight on them
}

// skimage.feature.canny(mask, sigma) of n boolean images (n, H, W) u8 on the device -> edges (n, H, W) u8 on the device
int canny_mask_dev(Ctx *c, const uint8_t *m, int n, int H, int W, double sigma, uint8_t *e, hipStream_t s)
{
    const int r = gauss_radius(sigma, 4.0);
    const int Hp = H + 2 * r, Wp = W + 2 * r;
    const size_t npx = (size_t)n * H * W, npad = (size_t)n * Hp * Wp;
    DevScope A(c->ws_pool, s);
    double *pa = A.pooled<double>(npad), *pb = A.pooled<double>(npad), *pt = A.pooled<double>(npad);
    CannyWs cw{};
    cw.sm = A.pooled<double>(npx); cw.t0 = A.pooled<double>(npx); cw.is_ = A.pooled<double>(npx); cw.js = A.pooled<double>(npx); cw.mag = A.pooled<double>(npx);
    cw.low = A.pooled<uint8_t>(npx); cw.high = A.pooled<uint8_t>(npx); cw.L = A.pooled<int>(npx); cw.flag = A.pooled<int>(npx);
    double *tabs = A.pooled<double>(6);
    A.h2d(tabs, A.keep(std::vector<double>{-1.0, 0.0, 1.0, 1.0, 2.0, 1.0}), 6 * sizeof(double));
    cw.w_diff = tabs; cw.w_smooth = tabs + 3;
    if (!A.ok) return TMAT_E_HIP;
    // gaussian(x, sigma, mode='constant') of the image and of the all-ones mask (0.18.3 smooth_with_function_and_mask): zero padding
    // by the kernel radius makes the boundary mode irrelevant
    launch_wm_pad(m, n, H, W, r, pa, pb, s);
    const GaussTable &gt = gauss_table(c, sigma, 0, r);
    const double *w = table_dev(c, gt);
    if (!w) return TMAT_E_HIP;
    launch_corr1d_f64(pa, pt, (size_t)n, Hp, Wp, w, gt.r, gt.sym, EXT_NEAREST, s);
    launch_corr1d_f64(pt, pa, (size_t)n * Hp, Wp, 1, w, gt.r, gt.sym, EXT_NEAREST, s);
    launch_corr1d_f64(pb, pt, (size_t)n, Hp, Wp, w, gt.r, gt.sym, EXT_NEAREST, s);
    launch_corr1d_f64(pt, pb, (size_t)n * Hp, Wp, 1, w, gt.r, gt.sym, EXT_NEAREST, s);
    launch_wm_crop_div(pa, pb, n, H, W, r, cw.sm, s);
    if (canny_core_dev(n, H, W, cw, e, s)) { set_error("tmat_canny_mask: kernel launch failed"); return TMAT_E_HIP; }
    return A.finish();
}

// ---- batch entry point of the branch: K stacks per pass, the host graph stage of pass p - 1 beside the device stages of pass p ----------

// Device bytes one stack of a pass holds at the pass's peak, from the blocks the stages take (DevScope::pooled in tmat_analyze_stack_batch,
// stack_prepare_dev, stack_resize_aa_dev, vessel_field_dev, the DMT front end).  Two phases never overlap, the larger one counts:
//   prepare   u16 stack, prepared volume, field + the per-slice gaussian's f64 plane, the zoomed f64 volume and the resize's two f64 planes
//   field     u16 stack, prepared volume, field + nine (Z - 1) f32 volumes, the 2-D planes of canny / medial axis / mask stages, then the tail
// The three Z H W f64 planes of the prepare phase dominate for any stack larger than its field.
size_t stack_pass_bytes(int Z, int H, int W, int fh, int fw)
{
    const size_t nin = (size_t)Z * H * W, npx = (size_t)fh * fw, nE = dmt_edge_count(fh, fw);
    const size_t held = nin * 2 + (size_t)Z * npx * 4 + npx * 4 + (size_t)H * W * 3;      // + projection and its picture
    const size_t prepare = nin * 8 * 3 + (size_t)Z * npx * 8;
    const size_t planes = npx * (4 * 4 + 5 * 8 + 2 + 2 * 4 + 5 + 8 + 4 + 6 * 8) + morph_workspace_bytes(1, fh, fw) + thin_workspace_bytes(1, fh, fw) + npx * 8;
    const size_t field = (size_t)(Z - 1) * npx * 4 * 9 + planes;
    const size_t tail = npx * 4 + nE * (4 + 1 + 4) + dmt_workspace_bytes(1, fh, fw) + dmt_sweep_workspace_bytes(1, fh, fw);
    return held + std::max(prepare, std::max(field, tail));
}

// stacks per pass: min(n, TMAT_STACK_PASS_MAX, budget / bytes per stack), at least 1; pass_stacks > 0 overrides
int stack_pass_count(int n, size_t bytes_per_stack, int pass_stacks)
{
    if (pass_stacks > 0) return std::max(1, std::min(n, pass_stacks));
    const size_t fit = bytes_per_stack ? (size_t)TMAT_STACK_PASS_BUDGET / bytes_per_stack : (size_t)TMAT_STACK_PASS_MAX;
    return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)n, TMAT_STACK_PASS_MAX), fit));
}

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// pinned result buffers of one pass slot: what the host graph stage reads while the next pass fills the other slot
struct StackSlot { float *f255; int32_t *ids; int *m; uint8_t *kind; float *pers; };

bool ensure_stack_slots(Ctx *c, int K, size_t npx, size_t nE, StackSlot sl[2])
{
    const size_t need[5] = {(size_t)K * npx * 4, (size_t)K * nE * 4, (size_t)K * sizeof(int), (size_t)K * nE, (size_t)K * nE * 4};
    bool fits = c->stack_host.ents.size() == 10;
    for (int i = 0; fits && i < 10; i++) fits = c->stack_host.ents[i].bytes >= need[i % 5];
    if (!fits) {
        c->stack_host.free_all();
        for (int i = 0; i < 10; i++) if (!c->stack_host.pinned(need[i % 5], "hipHostMalloc(stack pass results)")) { c->stack_host.free_all(); return false; }
    }
    for (int q = 0; q < 2; q++) {
        const WsEnt *e = &c->stack_host.ents[5 * q];
        sl[q] = StackSlot{(float *)e[0].p, (int32_t *)e[1].p, (int *)e[2].p, (uint8_t *)e[3].p, (float *)e[4].p};
    }
    return true;
}

struct StackJob {
    std::thread th;
    std::atomic<int> rc{0};
    void join() { if (th.joinable()) th.join(); }
};

// The tree request of a call (tmat_stack_opts.bars_out ...): the host graph stage calls tmat_morse_tree instead of tmat_morse_stats and
// leaves the segments of its (pair, stack) items here; the pass loop rasterises them over the pass's max projections, which stay in
// HBM in one of three slots (proj) until then.  Everything on the device is enqueued by the calling thread on the handle's stream,
// in order with the passes' own stages: a render kernel never runs beside the DMT sweep kernel, whose barrier between workgroups counts
// on having the chip.
struct StackTree {
    double sf;                      // compute_branches.py:437: W / fw
    double *bars_out; int cap_b; int *n_bars; uint8_t *rgb_out;     // caller's, whole call
    Canvas cv;
    uint16_t *proj[3];              // (K, H, W) u16 each, device
    OverlayWs ws;
    std::vector<std::vector<double>> segs[2];       // per result slot: (n_thresh, k) items of the pass
    std::vector<std::vector<int32_t>> branch[2];
};

// host graph stage of one pass: DMT collect + MorseGraph statistics of every (threshold pair, stack) on the shared worker threads
// rows: the call's rows (n_thresh, n); the pass's stacks are i0 .. i0 + k of every pair
void stack_pass_host(const StackSlot sl, int slot, int i0, int k, int fh, int fw, const tmat_stack_opts o, const uint8_t *pruning, bool sweep_dev, tmat_row *rows,
                     int n, StackTree *tree, StackJob *job, double *host_ms)
{
    const double t0 = now_ms();
    const size_t npx = (size_t)fh * fw, nE = dmt_edge_count(fh, fw);
    if (tree) { tree->segs[slot].assign((size_t)o.n_thresh * k, {}); tree->branch[slot].assign((size_t)o.n_thresh * k, {}); }
    parallel_images(o.n_thresh * k, [&](int it) {
        const int t = it / k, i = it - t * k;
        const int cap_v = (int)npx + 4, cap_e = 3 * (int)npx + 4;
        std::vector<int32_t> V((size_t)cap_v * 2), E((size_t)cap_e * 2);
        int nv = 0, ne = 0;
        int rc = dmt_graph_host_sorted(sl.f255 + i * npx, fh, fw, o.thresh[2 * t], o.thresh[2 * t + 1], sl.ids + i * nE, sl.m[i], V.data(), cap_v, E.data(),
                                       cap_e, &nv, &ne, sweep_dev ? sl.kind + i * nE : nullptr, sweep_dev ? sl.pers + i * nE : nullptr);
        const size_t at = (size_t)t * n + i0 + i;
        tmat_row *row = rows + at;
        const uint8_t *pm = pruning ? pruning + i * npx : nullptr;
        if (!rc && !tree)
            rc = tmat_morse_stats(V.data(), nv, E.data(), ne, fh, fw, o.smoothing_window_px, o.min_branch_length_px, o.max_branch_length_px, o.remove_isolated,
                                  pm, &row->count, &row->total_px, &row->avg_px, nullptr, 0);
        if (!rc && tree)
            rc = morse_tree_item(V.data(), nv, E.data(), ne, fh, fw, o.smoothing_window_px, o.min_branch_length_px, o.max_branch_length_px, o.remove_isolated,
                                 pm, tree->sf, &row->count, &row->total_px, &row->avg_px, tree->segs[slot][it], tree->branch[slot][it],
                                 tree->bars_out + at * tree->cap_b * 2, tree->cap_b, tree->n_bars + at);
        if (rc) job->rc = rc;
    });
    *host_ms = now_ms() - t0;
}

// the overlays of pass p (its host job has ended): pair by pair over the pass's projections, copied to the caller's (n_thresh, n, vh, vw, 3)
int stack_pass_render(StackTree &tr, int p, int K, int n, int n_thresh, int H, int W, hipStream_t s)
{
    const int slot = p & 1, i0 = p * K, k = std::min(K, n - i0);
    const size_t cper = (size_t)tr.cv.vh * tr.cv.vw * 3;
    const uint16_t *bg = tr.proj[p % 3];
    if (overlay_minmax_dev(bg, 0, k, H, W, tr.ws.dmm, s)) { set_error("tmat_analyze_stack_batch (tree): min-max launch failed"); return TMAT_E_HIP; }
    for (int t = 0; t < n_thresh; t++) {
        std::vector<OverlaySeg> ss;
        std::vector<int> off;
        int rc = overlay_pair_dev(bg, 0, k, H, W, tr.cv, &tr.segs[slot][(size_t)t * k], &tr.branch[slot][(size_t)t * k], tr.ws, ss, off,
                                  tr.rgb_out + ((size_t)t * n + i0) * cper, "tmat_analyze_stack_batch (tree)", s);
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = TMAT_E_HIP;       // the pair's canvases and tables are reused by the next pair
        if (rc) return rc;
    }
    return TMAT_OK;
}

bool hessian_ok(int h) { return h == TMAT_SATO_GAUSSIAN_DERIVATIVES || h == TMAT_SATO_GRADIENT; }

}  // namespace

// stacks_on_dev: `stacks` is device memory (tmat_analyze_stack_batch_dev); a pass then copies its stacks device to device into the block
// the per-slice gaussian overwrites, so the caller's buffer is only ever read
int analyze_stack_batch(Ctx *c, const uint16_t *stacks, bool stacks_on_dev, int n, int Z, int H, int W, const tmat_stack_opts &o, tmat_row *rows)
{
    const int fh = (int)std::nearbyint((double)H * ((double)o.ds_width / (double)W)), fw = (int)std::nearbyint((double)W * ((double)o.ds_width / (double)W));
    if (fh < 2 || fw < 2) { set_error("tmat_analyze_stack_batch: downsampled shape is empty"); return TMAT_E_ARG; }
    const size_t nin = (size_t)Z * H * W, hw = (size_t)H * W, npx = (size_t)fh * fw, nE = dmt_edge_count(fh, fw);
    const int K = stack_pass_count(n, stack_pass_bytes(Z, H, W, fh, fw), o.pass_stacks), P = (n + K - 1) / K;
    StackSlot slots[2];
    if (!ensure_stack_slots(c, K, npx, nE, slots)) return TMAT_E_HIP;
    for (int t = 0; t < o.n_thresh; t++)
        for (int i = 0; i < n; i++) { tmat_row &r = rows[(size_t)t * n + i]; r.index = o.first_index + i; r.count = 0; r.total_px = 0; r.avg_px = 0; }
    const bool sweep_dev = c->dmt_sweep_device;
    hipStream_t s = c->stream;
    // the tree request: scratch for the whole call, taken before any pass is in flight (the job threads never touch the pool)
    DevScope TA(c->ws_pool, s);
    StackTree tr{}, *tree = nullptr;
    if (o.bars_out) {
        tree = &tr;
        tr.sf = (double)W / (double)fw;
        tr.bars_out = o.bars_out; tr.cap_b = o.cap_b; tr.n_bars = o.n_bars; tr.rgb_out = o.rgb_out;
        for (size_t r = 0; r < (size_t)o.n_thresh * n; r++) o.n_bars[r] = 0;
        if (o.rgb_out) {
            if (!canvas_of(H, W, o.vis_width, tr.cv)) { set_error("tmat_analyze_stack_batch (tree): empty canvas"); return TMAT_E_ARG; }
            const size_t cper = (size_t)tr.cv.vh * tr.cv.vw * 3;
            for (uint16_t *&pr : tr.proj) pr = TA.pooled<uint16_t>((size_t)K * hw);
            tr.ws.seg_cap = (size_t)K * npx;
            tr.ws.dseg = TA.pooled<OverlaySeg>(tr.ws.seg_cap);
            tr.ws.dmm = TA.pooled<float>(4 * (size_t)K);
            tr.ws.doff = TA.pooled<int>((size_t)K + 1);
            tr.ws.drgb = TA.pooled<uint8_t>((size_t)K * cper);
            if (!TA.ok) return TMAT_E_HIP;
        }
    }
    const bool render = tree && o.rgb_out;
    StackJob jobs[2];
    std::vector<double> gpu_ms(P, 0.0), host_ms(P, 0.0);
    int rc = TMAT_OK;
    for (int p = 0; p < P && !rc; p++) {
        const int slot = p & 1, i0 = p * K, k = std::min(K, n - i0);
        const double t0 = now_ms();
        // every device stage of the pass in order on the handle's stream: passes never run side by side (the DMT sweep kernel's barrier
        // between workgroups counts on having the chip), the overlap is with the HOST stage of the pass before
        DevScope A(c->ws_pool, s);
        uint16_t *ds = stacks_on_dev ? A.pooled<uint16_t>((size_t)k * nin) : A.pooled_from(stacks + (size_t)i0 * nin, (size_t)k * nin);
        if (stacks_on_dev && A.ok) A.check(hipMemcpyAsync(ds, stacks + (size_t)i0 * nin, (size_t)k * nin * sizeof(uint16_t), hipMemcpyDeviceToDevice, s), "D2D");
        float *vol = A.pooled<float>((size_t)k * Z * npx), *field = A.pooled<float>((size_t)k * npx);
        if (!A.ok) { rc = TMAT_E_HIP; break; }
        void *mm = (o.proj_pic_out || o.field_pic_out) ? A.pooled_bytes(vis_scratch_bytes(k)) : nullptr;
        if (o.proj_pic_out) {
            // compute_branches.py:228-229: save_vis of the max projection, taken before the per-slice gaussian overwrites the stack
            uint16_t *proj = A.pooled<uint16_t>((size_t)k * hw);
            uint8_t *pic = A.pooled<uint8_t>((size_t)k * hw);
            if (!A.ok) { rc = TMAT_E_HIP; break; }
            double *lo = vis_scratch_lo(mm, k);
            if (zproj_dev(ds, k, Z, H, W, TMAT_ZPROJ_MAX, proj, s) || vis_minmax_dev(proj, TMAT_PIC_U16, k, hw, mm, s) ||
                vis_picture_dev(proj, TMAT_PIC_U16, k, hw, lo, lo + k, pic, s)) { set_error("tmat_analyze_stack_batch: projection picture failed"); rc = TMAT_E_HIP; break; }
            A.d2h(o.proj_pic_out + (size_t)i0 * hw, pic, (size_t)k * hw);
        }
        // the tree overlays' background, likewise before the gaussian; slot p % 3: pass p - 2 is drawn further down, after this is queued
        if (render && zproj_dev(ds, k, Z, H, W, TMAT_ZPROJ_MAX, tr.proj[p % 3], s)) { set_error("tmat_analyze_stack_batch (tree): projection failed"); rc = TMAT_E_HIP; break; }
        rc = stack_prepare_dev(c, ds, k, Z, H, W, fh, fw, vol, s);
        if (!rc) rc = vessel_field_dev(c, vol, k, Z, fh, fw, o.hessian, field, nullptr, s);
        if (rc) break;
        if (o.fields_out) A.d2h(o.fields_out + (size_t)i0 * npx, field, (size_t)k * npx * 4);
        if (o.field_pic_out) {      // :303 vesselness_image.png
            uint8_t *pic = A.pooled<uint8_t>((size_t)k * npx);
            if (!A.ok) { rc = TMAT_E_HIP; break; }
            double *lo = vis_scratch_lo(mm, k);
            if (vis_minmax_dev(field, TMAT_PIC_F32, k, npx, mm, s) || vis_picture_dev(field, TMAT_PIC_F32, k, npx, lo, lo + k, pic, s)) {
                set_error("tmat_analyze_stack_batch: field picture failed"); rc = TMAT_E_HIP; break;
            }
            A.d2h(o.field_pic_out + (size_t)i0 * npx, pic, (size_t)k * npx);
        }
        // device front end of the tail for the k fields: rescale to 0..255 per image (:419), lower-star sort, the two persistence sweeps
        float *f255 = A.pooled<float>((size_t)k * npx), *mnmx = A.pooled<float>(2 * (size_t)k);
        int32_t *ids = A.pooled<int32_t>((size_t)k * nE);
        int *m = A.pooled<int>(k);
        void *dws = A.pooled_bytes(dmt_workspace_bytes(k, fh, fw));
        uint8_t *dkind = sweep_dev ? A.pooled<uint8_t>((size_t)k * nE) : nullptr;
        float *dpers = sweep_dev ? A.pooled<float>((size_t)k * nE) : nullptr;
        void *sws = sweep_dev ? A.pooled_bytes(dmt_sweep_workspace_bytes(k, fh, fw)) : nullptr;
        if (!A.ok) { rc = TMAT_E_HIP; break; }
        launch_rescale255(field, k, (int)npx, mnmx, mnmx + k, f255, s);
        if (dmt_sorted_edges_dev(f255, k, fh, fw, dws, ids, m, s)) { set_error("tmat_analyze_stack_batch: DMT front end failed"); rc = TMAT_E_HIP; break; }
        if (sweep_dev && dmt_sweeps_dev(f255, ids, m, k, fh, fw, sws, dkind, dpers, s)) { set_error("tmat_analyze_stack_batch: device sweeps failed"); rc = TMAT_E_HIP; break; }
        // the slot's host buffers are free once the job of the pass before last has ended
        jobs[slot].join();
        if (jobs[slot].rc) { rc = jobs[slot].rc; break; }
        if (render && p >= 2 && (rc = stack_pass_render(tr, p - 2, K, n, o.n_thresh, H, W, s))) break;
        const StackSlot &sl = slots[slot];
        A.d2h(sl.f255, f255, (size_t)k * npx * 4);
        A.d2h(sl.ids, ids, (size_t)k * nE * sizeof(int32_t));
        A.d2h(sl.m, m, (size_t)k * sizeof(int));
        if (sweep_dev) { A.d2h(sl.kind, dkind, (size_t)k * nE); A.d2h(sl.pers, dpers, (size_t)k * nE * sizeof(float)); }
        if (A.finish()) { rc = TMAT_E_HIP; break; }
        gpu_ms[p] = now_ms() - t0;
        jobs[slot].th = std::thread(stack_pass_host, sl, slot, i0, k, fh, fw, o, o.pruning_masks ? o.pruning_masks + (size_t)i0 * npx : nullptr, sweep_dev, rows, n,
                                    tree, &jobs[slot], &host_ms[p]);
    }
    for (StackJob &j : jobs) { j.join(); if (j.rc && !rc) rc = j.rc; }
    // the overlays of the last two passes (the loop drew pass p - 2 during pass p); every host job has ended
    for (int p = std::max(0, P - 2); render && !rc && p < P; p++) rc = stack_pass_render(tr, p, K, n, o.n_thresh, H, W, s);
    c->stack_trace.clear();
    for (int p = 0; p < P; p++) c->stack_trace.push_back({gpu_ms[p], host_ms[p]});
    static const bool trace = [] { const char *e = getenv("TMAT_TRACE"); return e && atoi(e) > 0; }();
    if (trace)
        for (int p = 0; p < P; p++)
            fprintf(stderr, "[tmat] stack pass %d (%d stacks): device stages %.1f ms, host graph stage %.1f ms\n", p, std::min(K, n - p * K), gpu_ms[p], host_ms[p]);
    return rc;
}

}  // namespace tmat

using namespace tmat;

extern "C" {

int tmat_gaussian_f32(tmat_handle hd, const float *x, int d0, int d1, int d2, double sigma, int mode, float *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !x || !out || d0 < 1 || d1 < 1 || d2 < 1 || !(sigma > 0) || mode < 0 || mode > 2) { set_error("tmat_gaussian_f32: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)d0 * d1 * d2;
    hipStream_t s = c->stream;
    DevScope A(c->ws_pool, s);
    float *a = A.pooled_from(x, n), *b = A.pooled<float>(n);
    if (!A.ok) return TMAT_E_HIP;
    // ndi.gaussian_filter: every axis in order (the caller folds leading axes of length 1 away by passing d0 = 1 -> two passes)
    float *src = a, *dst = b;
    if (d0 > 1) { if (!gauss_pass_f32(c, src, dst, Pass{sigma, 0, d0, d1 * d2, 1}, 4.0, mode, s)) return TMAT_E_HIP; std::swap(src, dst); }
    if (!gauss_pass_f32(c, src, dst, Pass{sigma, 0, d1, d2, (size_t)d0}, 4.0, mode, s)) return TMAT_E_HIP;
    std::swap(src, dst);
    if (!gauss_pass_f32(c, src, dst, Pass{sigma, 0, d2, 1, (size_t)d0 * d1}, 4.0, mode, s)) return TMAT_E_HIP;
    A.d2h(out, dst, n * 4);
    return A.finish();
}

/* well_mask_generation.auto_threshold_well (reference :236-277) on the device: img (H, W) -> thresholded, eroded mask u8.
 * is_f64 = 0: a float32 image (what compute_branches.py hands over); 1: float64 (integer images after img_as_float) */
static int well_threshold(tmat_handle hd, const void *img, int is_f64, int H, int W, uint8_t *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !img || !out || H < 20 || W < 20 || (long long)H * W > (1LL << 28)) { set_error("tmat_well_threshold: bad argument (images of at least 20 x 20)"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = (size_t)H * W;
    DevScope A(c->ws_pool, s);
    uint8_t *er = A.pooled<uint8_t>(n);
    int rc;
    if (is_f64) {
        double *da = A.pooled_from((const double *)img, n);
        if (!A.ok) return TMAT_E_HIP;
        rc = well_threshold_dev(c, da, nullptr, 1, H, W, er, s);
    } else {
        float *a = A.pooled_from((const float *)img, n);
        if (!A.ok) return TMAT_E_HIP;
        rc = well_threshold_dev(c, nullptr, a, 1, H, W, er, s);
    }
    if (rc) return rc;
    A.d2h(out, er, n);
    return A.finish();
}

int tmat_well_threshold(tmat_handle hd, const float *img, int H, int W, uint8_t *out) { return well_threshold(hd, img, 0, H, W, out); }
int tmat_well_threshold_f64(tmat_handle hd, const double *img, int H, int W, uint8_t *out) { return well_threshold(hd, img, 1, H, W, out); }

static bool canny_mask_args_ok(int n, int H, int W, double sigma) { return n >= 1 && H >= 3 && W >= 3 && sigma > 0 && sigma <= 16 && (long long)n * H * W <= (1LL << 26); }

/* skimage.feature.canny(mask, sigma) of boolean images with the default thresholds (reference calls:
 * well_mask_generation.py:165, :201): n masks (n, H, W) u8 -> edges u8, each as from a call of its own */
int tmat_canny_mask_batch(tmat_handle hd, const uint8_t *masks, int n, int H, int W, double sigma, uint8_t *edges)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !masks || !edges || !canny_mask_args_ok(n, H, W, sigma)) { set_error("tmat_canny_mask: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t npx = (size_t)n * H * W;
    DevScope A(c->ws_pool, s);
    uint8_t *m = A.pooled_from(masks, npx), *e = A.pooled<uint8_t>(npx);
    if (!A.ok) return TMAT_E_HIP;
    int rc = canny_mask_dev(c, m, n, H, W, sigma, e, s);
    if (rc) return rc;
    A.d2h(edges, e, npx);
    return A.finish();
}

int tmat_canny_mask(tmat_handle hd, const uint8_t *mask, int H, int W, double sigma, uint8_t *edges) { return tmat_canny_mask_batch(hd, mask, 1, H, W, sigma, edges); }

int tmat_well_small_shape(int h, int w, int *small_h, int *small_w)
{
    if (h < 1 || w < 1 || !small_h || !small_w) { set_error("tmat_well_small_shape: bad argument"); return TMAT_E_ARG; }
    well_small_shape(h, w, small_h, small_w);
    return TMAT_OK;
}

int tmat_stack_well_front_dev(tmat_handle hd, const uint16_t *stacks_dev, int n, int Z, int H, int W, int out_h, int out_w, double *proj_aa_out,
                              uint8_t *thresh_small, uint8_t *border_small)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !stacks_dev || !thresh_small || !border_small || n < 1 || Z < 1 || H < 1 || W < 1 || out_h < 20 || out_w < 20 ||
        (long long)n * out_h * out_w > (1LL << 26)) {
        set_error("tmat_stack_well_front_dev: bad argument (n >= 1 stacks, a field of at least 20 x 20)");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int sh, sw;
    well_small_shape(out_h, out_w, &sh, &sw);
    if (sh < 3 || sw < 3) { set_error("tmat_stack_well_front_dev: the small mask is below 3 x 3"); return TMAT_E_ARG; }
    const size_t hw = (size_t)H * W, npx = (size_t)out_h * out_w, spx = (size_t)sh * sw;
    DevScope A(c->ws_pool, s);
    uint16_t *proj = A.pooled<uint16_t>((size_t)n * hw);
    double *aa = A.pooled<double>((size_t)n * npx);
    uint8_t *th = A.pooled<uint8_t>((size_t)n * npx), *small = A.pooled<uint8_t>((size_t)n * spx), *border = A.pooled<uint8_t>((size_t)n * spx);
    if (!A.ok) return TMAT_E_HIP;
    // compute_branches.py:227-238: max projection, anti-aliased resize -- one stack is one image with its own clip range
    if (zproj_dev(stacks_dev, n, Z, H, W, TMAT_ZPROJ_MAX, proj, s)) { set_error("tmat_stack_well_front_dev: projection failed"); return TMAT_E_HIP; }
    int rc = stack_resize_aa_dev(c, proj, n, 1, H, W, out_h, out_w, aa, nullptr, s);
    if (rc) return rc;
    A.d2h(proj_aa_out, aa, (size_t)n * npx * 8);
    // generate_well_mask :156-170: threshold, nearest resize to <= 200 px, border of the small mask
    rc = well_threshold_dev(c, aa, nullptr, n, out_h, out_w, th, s);
    if (rc) return rc;
    launch_resize_nearest_u8(th, n, out_h, out_w, sh, sw, small, s);
    rc = canny_mask_dev(c, small, n, sh, sw, 1.0, border, s);
    if (rc) return rc;
    launch_wm_border(small, n, sh, sw, border, s);
    A.check(hipGetLastError(), "tmat_stack_well_front_dev: kernel launch");
    A.d2h(thresh_small, small, (size_t)n * spx);
    A.d2h(border_small, border, (size_t)n * spx);
    return A.finish();
}

int tmat_cell_well_front_dev(tmat_handle hd, const uint16_t *small_dev, int n, int hh, int ww, int src_bits, uint8_t *thresh_small, uint8_t *border_small)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !small_dev || !thresh_small || !border_small || n < 1 || hh < 20 || ww < 20 || (long long)n * hh * ww > (1LL << 26)) {
        set_error("tmat_cell_well_front_dev: bad argument (n >= 1 images of at least 20 x 20, n hh ww <= 2^26)");
        return TMAT_E_ARG;
    }
    if (src_bits != 8 && src_bits != 16) { set_error("tmat_cell_well_front_dev: src_bits must be 8 or 16"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int sh, sw;
    well_small_shape(hh, ww, &sh, &sw);
    if (sh < 3 || sw < 3) { set_error("tmat_cell_well_front_dev: the small mask is below 3 x 3"); return TMAT_E_ARG; }
    const size_t npx = (size_t)hh * ww, spx = (size_t)sh * sw;
    DevScope A(c->ws_pool, s);
    double *f = A.pooled<double>((size_t)n * npx);
    uint8_t *th = A.pooled<uint8_t>((size_t)n * npx), *small = A.pooled<uint8_t>((size_t)n * spx), *border = A.pooled<uint8_t>((size_t)n * spx);
    if (!A.ok) return TMAT_E_HIP;
    // auto_threshold_well of an integer image: gaussian() converts with img_as_float first
    launch_wm_unit_f64(small_dev, (size_t)n * npx, src_bits == 8 ? 1.0 / 255.0 : 1.0 / 65535.0, f, s);
    // generate_well_mask :156-170: threshold, nearest resize to <= 200 px, border of the small mask
    int rc = well_threshold_dev(c, f, nullptr, n, hh, ww, th, s);
    if (rc) return rc;
    launch_resize_nearest_u8(th, n, hh, ww, sh, sw, small, s);
    rc = canny_mask_dev(c, small, n, sh, sw, 1.0, border, s);
    if (rc) return rc;
    launch_wm_border(small, n, sh, sw, border, s);
    A.check(hipGetLastError(), "tmat_cell_well_front_dev: kernel launch");
    A.d2h(thresh_small, small, (size_t)n * spx);
    A.d2h(border_small, border, (size_t)n * spx);
    return A.finish();
}

int tmat_sato_batch(tmat_handle hd, const float *imgs, int n, int hh, int ww, const double *sigmas, int n_sigmas, int hessian, float *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !imgs || !out || n < 0 || hh < 2 || ww < 2 || n_sigmas < 0 || (n_sigmas && !sigmas) ||
        (hessian != TMAT_SATO_GAUSSIAN_DERIVATIVES && hessian != TMAT_SATO_GRADIENT)) { set_error("tmat_sato_batch: bad argument"); return TMAT_E_ARG; }
    for (int k = 0; k < n_sigmas; k++) if (!(sigmas[k] > 0)) { set_error("tmat_sato_batch: sigmas must be positive"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t total = (size_t)n * hh * ww;
    hipStream_t s = c->stream;
    DevScope A(c->ws_pool, s);
    float *raw = A.pooled_from(imgs, total), *x = A.pooled<float>(total), *best = A.pooled<float>(total), *bufs[7];
    for (float *&b : bufs) b = A.pooled<float>(total);
    if (!A.ok) return TMAT_E_HIP;
    launch_prep_single(raw, total, hessian == TMAT_SATO_GAUSSIAN_DERIVATIVES, x, s);
    if (!sato_dev(c, x, n, hh, ww, sigmas, n_sigmas, hessian, bufs, best, s)) { set_error("tmat_sato_batch: kernel launch failed"); return TMAT_E_HIP; }
    A.d2h(out, best, total * 4);
    return A.finish();
}

int tmat_stack_prepare(tmat_handle hd, const uint16_t *stack, int Z, int H, int W, int out_h, int out_w, float *vol)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !stack || !vol || Z < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) { set_error("tmat_stack_prepare: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t nin = (size_t)Z * H * W, nout = (size_t)Z * out_h * out_w;
    DevScope A(c->ws_pool, c->stream);
    uint16_t *ds = A.pooled_from(stack, nin);
    float *dv = A.pooled<float>(nout);
    if (!A.ok) return TMAT_E_HIP;
    int rc = stack_prepare_dev(c, ds, 1, Z, H, W, out_h, out_w, dv, c->stream);
    if (rc) return rc;
    A.d2h(vol, dv, nout * 4);
    return A.finish();
}

int tmat_vessel_field(tmat_handle hd, const float *vol, int Z, int hh, int ww, int hessian, float *field, const tmat_vessel_stages *stages)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !vol || !field || Z < 2 || hh < 2 || ww < 2 || (hessian != TMAT_SATO_GAUSSIAN_DERIVATIVES && hessian != TMAT_SATO_GRADIENT)) {
        set_error("tmat_vessel_field: bad argument");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t nvol = (size_t)Z * hh * ww, npx = (size_t)hh * ww;
    DevScope A(c->ws_pool, c->stream);
    float *dv = A.pooled_from(vol, nvol), *df = A.pooled<float>(npx);
    if (!A.ok) return TMAT_E_HIP;
    int rc = vessel_field_dev(c, dv, 1, Z, hh, ww, hessian, df, stages, c->stream);
    if (rc) return rc;
    A.d2h(field, df, npx * 4);
    return A.finish();
}

// common tail of analyze_img from the vesselness image in HBM: rescale_intensity(0..255) (:419), DMT graph, MorseGraph statistics
static int field_stats_dev(Ctx *c, const float *field, int fh, int fw, float t1, float t2, int smooth, int min_len, int max_len, int remove_isolated,
                           const uint8_t *pruning_mask, int64_t index, tmat_row *row, hipStream_t s)
{
    const size_t npx = (size_t)fh * fw, nE = dmt_edge_count(fh, fw);
    DevScope A(c->ws_pool, s);
    float *f255 = A.pooled<float>(npx), *mnmx = A.pooled<float>(2);
    int32_t *ids = A.pooled<int32_t>(nE);
    int *m = A.pooled<int>(1);
    void *dws = A.pooled_bytes(dmt_workspace_bytes(1, fh, fw));
    if (!A.ok) return TMAT_E_HIP;
    launch_rescale255(field, 1, (int)npx, mnmx, mnmx + 1, f255, s);
    float *f255_host = A.host<float>(npx);
    int32_t *ids_host = A.host<int32_t>(nE);
    int *m_host = A.host<int>();
    if (dmt_sorted_edges_dev(f255, 1, fh, fw, dws, ids, m, s)) { set_error("field stats: DMT front end failed"); return TMAT_E_HIP; }
    // the two persistence sweeps on the device as well (dmt_sweep_kernels.hip; TMAT_DMT_SWEEP_DEVICE=0: inside dmt_graph_host_sorted)
    uint8_t *kind_host = nullptr;
    float *pers_host = nullptr;
    if (c->dmt_sweep_device) {
        uint8_t *dkind = A.pooled<uint8_t>(nE);
        float *dpers = A.pooled<float>(nE);
        void *sws = A.pooled_bytes(dmt_sweep_workspace_bytes(1, fh, fw));
        if (!A.ok) return TMAT_E_HIP;
        if (dmt_sweeps_dev(f255, ids, m, 1, fh, fw, sws, dkind, dpers, s)) { set_error("field stats: device sweeps failed"); return TMAT_E_HIP; }
        A.d2h(kind_host = A.host<uint8_t>(nE), dkind, nE);
        A.d2h(pers_host = A.host<float>(nE), dpers, nE * sizeof(float));
    }
    A.d2h(f255_host, f255, npx * 4);
    A.d2h(ids_host, ids, nE * sizeof(int32_t));
    A.d2h(m_host, m, sizeof(int));
    if (A.finish()) return TMAT_E_HIP;
    const int cap_v = (int)npx + 4, cap_e = 3 * (int)npx + 4;
    std::vector<int32_t> V((size_t)cap_v * 2), E((size_t)cap_e * 2);
    int nv = 0, ne = 0;
    int rc = dmt_graph_host_sorted(f255_host, fh, fw, t1, t2, ids_host, *m_host, V.data(), cap_v, E.data(), cap_e, &nv, &ne, kind_host, pers_host);
    row->index = index; row->count = 0; row->total_px = 0; row->avg_px = 0;
    if (!rc)
        rc = tmat_morse_stats(V.data(), nv, E.data(), ne, fh, fw, smooth, min_len, max_len, remove_isolated, pruning_mask, &row->count, &row->total_px,
                              &row->avg_px, nullptr, 0);
    return rc;
}

int tmat_field_stats_pruned(tmat_handle hd, const float *field, int fh, int fw, float graph_thresh_1, float graph_thresh_2, int smoothing_window_px,
                            int min_branch_length_px, int max_branch_length_px, int remove_isolated, const uint8_t *pruning_mask, int64_t index,
                            tmat_row *row)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !field || !row || fh < 2 || fw < 2) { set_error("tmat_field_stats: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    DevScope A(c->ws_pool, c->stream);
    float *df = A.pooled_from(field, (size_t)fh * fw);
    if (!A.ok) return TMAT_E_HIP;
    return field_stats_dev(c, df, fh, fw, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px, remove_isolated,
                           pruning_mask, index, row, c->stream);
}

int tmat_field_stats(tmat_handle hd, const float *field, int fh, int fw, float graph_thresh_1, float graph_thresh_2, int smoothing_window_px,
                     int min_branch_length_px, int max_branch_length_px, int remove_isolated, int64_t index, tmat_row *row)
{
    return tmat_field_stats_pruned(hd, field, fh, fw, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px,
                                   remove_isolated, nullptr, index, row);
}

int tmat_resize_aa_u16(tmat_handle hd, const uint16_t *imgs, int n, int H, int W, int out_h, int out_w, double *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !imgs || !out || n < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) { set_error("tmat_resize_aa_u16: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t nin = (size_t)n * H * W, nout = (size_t)n * out_h * out_w;
    DevScope A(c->ws_pool, c->stream);
    uint16_t *ds = A.pooled_from(imgs, nin);
    double *dz = A.pooled<double>(nout);
    if (!A.ok) return TMAT_E_HIP;
    int rc = stack_resize_aa_dev(c, ds, 1, n, H, W, out_h, out_w, dz, nullptr, c->stream);      // one clip range over the n images, as ever
    if (rc) return rc;
    A.d2h(out, dz, nout * 8);
    return A.finish();
}

int tmat_analyze_stack(tmat_handle hd, const uint16_t *stack, int Z, int H, int W, int ds_width, int hessian, float graph_thresh_1,
                       float graph_thresh_2, int smoothing_window_px, int min_branch_length_px, int max_branch_length_px, int remove_isolated,
                       int64_t index, tmat_row *row, float *field_out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !stack || !row || Z < 2 || H < 2 || W < 2 || ds_width < 2 || (hessian != TMAT_SATO_GAUSSIAN_DERIVATIVES && hessian != TMAT_SATO_GRADIENT)) {
        set_error("tmat_analyze_stack: bad argument");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    // img_dsamp_res = round(shape * ds_width / width), half to even (compute_branches.py:218-222)
    const int fh = (int)std::nearbyint((double)H * ((double)ds_width / (double)W)), fw = (int)std::nearbyint((double)W * ((double)ds_width / (double)W));
    if (fh < 2 || fw < 2) { set_error("tmat_analyze_stack: downsampled shape is empty"); return TMAT_E_ARG; }
    const size_t nin = (size_t)Z * H * W, npx = (size_t)fh * fw;
    hipStream_t s = c->stream;
    DevScope A(c->ws_pool, s);
    uint16_t *ds = A.pooled_from(stack, nin);
    float *vol = A.pooled<float>((size_t)Z * npx), *field = A.pooled<float>(npx);
    if (!A.ok) return TMAT_E_HIP;
    int rc = stack_prepare_dev(c, ds, 1, Z, H, W, fh, fw, vol, s);
    if (!rc) rc = vessel_field_dev(c, vol, 1, Z, fh, fw, hessian, field, nullptr, s);
    if (rc) return rc;
    if (!A.d2h(field_out, field, npx * 4)) return TMAT_E_HIP;
    return field_stats_dev(c, field, fh, fw, graph_thresh_1, graph_thresh_2, smoothing_window_px, min_branch_length_px, max_branch_length_px,
                           remove_isolated, nullptr, index, row, s);
}

int tmat_stack_pass_plan(int n, int Z, int H, int W, int ds_width, int pass_stacks, int *stacks_per_pass, uint64_t *bytes_per_stack)
{
    if (n < 1 || Z < 2 || H < 2 || W < 2 || ds_width < 2 || pass_stacks < 0 || (!stacks_per_pass && !bytes_per_stack)) { set_error("tmat_stack_pass_plan: bad argument"); return TMAT_E_ARG; }
    const int fh = (int)std::nearbyint((double)H * ((double)ds_width / (double)W)), fw = (int)std::nearbyint((double)W * ((double)ds_width / (double)W));
    if (fh < 2 || fw < 2) { set_error("tmat_stack_pass_plan: downsampled shape is empty"); return TMAT_E_ARG; }
    const size_t b = stack_pass_bytes(Z, H, W, fh, fw);
    if (bytes_per_stack) *bytes_per_stack = b;
    if (stacks_per_pass) *stacks_per_pass = stack_pass_count(n, b, pass_stacks);
    return TMAT_OK;
}

static int analyze_stack_batch_entry(tmat_handle hd, const uint16_t *stacks, bool stacks_on_dev, int n, int Z, int H, int W, const tmat_stack_opts *o, tmat_row *rows)
{
    Ctx *c = (Ctx *)hd;
    static_assert(offsetof(tmat_stack_opts, vis_width) + sizeof(int) == TMAT_STACK_OPTS_SIZE_V1, "the first version of tmat_stack_opts ends with pass_stacks");
    if (!o || (o->size != (uint32_t)sizeof(tmat_stack_opts) && o->size != TMAT_STACK_OPTS_SIZE_V1)) { set_error("tmat_analyze_stack_batch: unknown tmat_stack_opts size"); return TMAT_E_ARG; }
    tmat_stack_opts full{};         // a caller of the first version: its fields, no tree request (what follows pass_stacks there is padding)
    std::memcpy(&full, o, o->size == TMAT_STACK_OPTS_SIZE_V1 ? offsetof(tmat_stack_opts, vis_width) : sizeof(tmat_stack_opts));
    o = &full;
    if (!c || !stacks || !rows || n < 1 || Z < 2 || H < 2 || W < 2 || o->ds_width < 2 || o->pass_stacks < 0) {
        set_error("tmat_analyze_stack_batch: bad argument (n >= 1 stacks of Z >= 2 slices)");
        return TMAT_E_ARG;
    }
    if (!hessian_ok(o->hessian)) { set_error("tmat_analyze_stack_batch: unknown hessian form"); return TMAT_E_ARG; }
    if (o->n_thresh < 1 || !o->thresh) { set_error("tmat_analyze_stack_batch: needs at least one threshold pair"); return TMAT_E_ARG; }
    if ((o->bars_out || o->n_bars || o->rgb_out) && (!o->bars_out || !o->n_bars || o->cap_b < 0 || (o->rgb_out && o->vis_width < 1))) {
        set_error("tmat_analyze_stack_batch: a tree request needs bars_out, n_bars, cap_b >= 0 and, with rgb_out, vis_width >= 1");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    return analyze_stack_batch(c, stacks, stacks_on_dev, n, Z, H, W, *o, rows);
}

int tmat_analyze_stack_batch(tmat_handle hd, const uint16_t *stacks, int n, int Z, int H, int W, const tmat_stack_opts *o, tmat_row *rows)
{
    return analyze_stack_batch_entry(hd, stacks, false, n, Z, H, W, o, rows);
}

int tmat_analyze_stack_batch_dev(tmat_handle hd, const uint16_t *stacks_dev, int n, int Z, int H, int W, const tmat_stack_opts *o, tmat_row *rows)
{
    return analyze_stack_batch_entry(hd, stacks_dev, true, n, Z, H, W, o, rows);
}

int tmat_vessel_field_batch(tmat_handle hd, const float *vols, int n, int Z, int hh, int ww, int hessian, float *fields, const tmat_vessel_stages *stages)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !vols || !fields || n < 1 || Z < 2 || hh < 2 || ww < 2 || !hessian_ok(hessian)) { set_error("tmat_vessel_field_batch: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t nvol = (size_t)n * Z * hh * ww, npx = (size_t)n * hh * ww;
    DevScope A(c->ws_pool, c->stream);
    float *dv = A.pooled_from(vols, nvol), *df = A.pooled<float>(npx);
    if (!A.ok) return TMAT_E_HIP;
    int rc = vessel_field_dev(c, dv, n, Z, hh, ww, hessian, df, stages, c->stream);
    if (rc) return rc;
    A.d2h(fields, df, npx * 4);
    return A.finish();
}

int tmat_debug_stack_trace(tmat_handle hd, int cap, int *n_pass, double *gpu_ms, double *host_ms)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !n_pass || cap < 0 || (cap > 0 && (!gpu_ms || !host_ms))) { set_error("tmat_debug_stack_trace: bad argument"); return TMAT_E_ARG; }
    *n_pass = (int)c->stack_trace.size();
    for (int i = 0; i < *n_pass && i < cap; i++) { gpu_ms[i] = c->stack_trace[i].first; host_ms[i] = c->stack_trace[i].second; }
    return TMAT_OK;
}

int tmat_host_gaussian_kernel1d(double sigma, int order, int radius, double *weights)
{
    if (!weights || !(sigma > 0) || order < 0 || order > 1 || radius < 0) { set_error("tmat_host_gaussian_kernel1d: bad argument"); return TMAT_E_ARG; }
    std::vector<double> w;
    gaussian_kernel1d(sigma, order, radius, w);
    std::memcpy(weights, w.data(), w.size() * sizeof(double));
    return TMAT_OK;
}

}  // extern "C"
