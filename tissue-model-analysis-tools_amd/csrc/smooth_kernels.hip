// Smooth tiling around ANY predictor, for any window size and subdivision count, as a device stage.
//
// Reference: fl_tissue_model_tools/smooth_tiled_predictions.py
//   _pad_img :68-79, _rotate_mirror_do :95-113, _windowed_subdivs :136-192 (the predictor calls :174-182 stay with the caller),
//   _recreate_from_subdivs :195-217, _rotate_mirror_undo :116-133, driver :220-267.
//
// blend_kernels.hip is the same driver specialised to subdivisions = 2 with the library's own network between the two gathers, and
// its kernels stay as they are (a path compiled into a hot kernel costs launches that never take it).  Here
//   aug  = int(round(ws (1 - 1 / s)))   Python's round: halves to even
//   step = int(ws / s)                  need not divide the frame: the strip behind the last tile of an orientation contributes 0.0
//   tiles:  patch(g, a, b)[p][q] = D4_g(pad(x))[a step + p][b step + q]                                  (f32 copy)
//   blend:  out[y][x] = ( sum_g ( sum_{tiles (a, b) of g covering the pixel, a then b ascending}
//                                    f64(pred) * (w[p] * w[q]) ) / (s s) ) / 8
// with the reference's f64 operation order: sequential adds from 0.0, the window product formed first, an IEEE division by s s (9 is
// no power of two), the eight orientations added in order.  No atomics, no canvases.  Compiled with -ffp-contract=off.
#include "tmat_ctx.h"

#include <climits>
#include <cmath>

namespace tmat {

bool smooth_geom(int hh, int ww, int ws, int sub, SmoothGeom &g)
{
    if (ws < 4 || sub < 2 || sub > ws || hh < 1 || ww < 1 || hh > (1 << 19) || ww > (1 << 19) || ws > (1 << 15)) {
        set_error("smooth tiling: needs 4 <= window_size <= 32768, 2 <= subdivisions <= window_size and an image of 1 .. 524288 pixels a side");
        return false;
    }
    g.hh = hh; g.ww = ww; g.ws = ws; g.sub = sub;
    g.step = ws / sub;                                                      // int(window_size / subdivisions)
    g.aug = (int)std::nearbyint((double)ws * (1.0 - 1.0 / (double)sub));    // default rounding mode: halves to even, as Python's round
    g.Hp = hh + 2 * g.aug; g.Wp = ww + 2 * g.aug;
    if (g.Hp < ws || g.Wp < ws) { set_error("smooth tiling: the padded image is smaller than the window"); return false; }
    const int cntH = (g.Hp - ws) / g.step + 1, cntW = (g.Wp - ws) / g.step + 1;
    g.na[0] = cntH; g.nb[0] = cntW;     // even rotations: the frame is Hp x Wp
    g.na[1] = cntW; g.nb[1] = cntH;     // odd rotations: Wp x Hp
    const long long total = 8LL * cntH * cntW;
    if (total > INT_MAX / 2) { set_error("smooth tiling: too many tiles"); return false; }
    int off = 0;
    for (int k = 0; k < 8; k++) { g.tile_off[k] = off; off += g.na[k & 1] * g.nb[k & 1]; }
    g.n_tiles = off;
    return true;
}

// frame coords (u, v) of orientation g -> padded-image coords (y, x), and back (np.rot90 k = g & 3 of the image, mirrored first for g >= 4)
__device__ __forceinline__ void smooth_frame_to_pad(int g, int u, int v, int Hp, int Wp, int &y, int &x)
{
    const int k = g & 3;
    int xp;
    if (k == 0) { y = u; xp = v; }
    else if (k == 1) { y = v; xp = Wp - 1 - u; }
    else if (k == 2) { y = Hp - 1 - u; xp = Wp - 1 - v; }
    else { y = Hp - 1 - v; xp = u; }
    x = (g & 4) ? Wp - 1 - xp : xp;
}
__device__ __forceinline__ void smooth_pad_to_frame(int g, int y, int x, int Hp, int Wp, int &u, int &v)
{
    const int k = g & 3;
    const int xp = (g & 4) ? Wp - 1 - x : x;
    if (k == 0) { u = y; v = xp; }
    else if (k == 1) { u = Wp - 1 - xp; v = y; }
    else if (k == 2) { u = Hp - 1 - y; v = Wp - 1 - xp; }
    else { u = xp; v = Hp - 1 - y; }
}

// grid: count * bpt workgroups, bpt = ceil(ws ws / 256) per tile; the launcher keeps first + count <= n_tiles
__global__ __launch_bounds__(256) void smooth_tiles_kernel(const float *__restrict__ x, const float *__restrict__ padval, SmoothGeom gm,
                                                           int first, int bpt, float *__restrict__ patches)
{
    const int slot = blockIdx.x / bpt;
    const int pix = (blockIdx.x - slot * bpt) * 256 + threadIdx.x;
    if (pix >= gm.ws * gm.ws) return;
    const int tile = first + slot;
    int g = 7;
#pragma unroll
    for (int k = 1; k < 8; k++) if (tile < gm.tile_off[k]) { g = k - 1; break; }
    const int tl = tile - gm.tile_off[g];
    const int nb = gm.nb[g & 1];
    const int a = tl / nb, b = tl - a * nb;
    const int p = pix / gm.ws, q = pix - p * gm.ws;
    int y, xx;
    smooth_frame_to_pad(g, a * gm.step + p, b * gm.step + q, gm.Hp, gm.Wp, y, xx);
    y -= gm.aug; xx -= gm.aug;
    float v = padval[0];
    if (y >= 0 && y < gm.hh && xx >= 0 && xx < gm.ww) v = x[(size_t)y * gm.ww + xx];
    patches[((size_t)slot * gm.ws + p) * gm.ws + q] = v;
}
void launch_smooth_tiles(const float *x, const float *padval, const SmoothGeom &g, int first, int count, float *patches, hipStream_t s)
{
    const int bpt = (g.ws * g.ws + 255) / 256;
    const int per = std::max(1, (1 << 30) / bpt);       // tiles of one launch: the grid stays below 2^31 workgroups
    for (int i = 0; i < count; i += per) {
        const int k = std::min(per, count - i);
        hipLaunchKernelGGL(smooth_tiles_kernel, dim3((unsigned)k * bpt), dim3(256), 0, s, x, padval, g, first + i, bpt,
                           patches + (size_t)i * g.ws * g.ws);
    }
}

// One output pixel per thread, a 16 x 16 pixel block per workgroup (a wave: 4 rows of 16, four 128-byte stores).  In the four odd
// orientations a pixel row of the image is a COLUMN of the tiles: 64 lanes along x read one line per lane there, the square block reads
// 16 short lines in either kind of orientation.  Measured at 640 x 640, ws 320 against the 64 x 4 form: 0.036 ms against 0.052 ms
// at subdivisions 2, 0.113 ms against 0.197 ms at 4, the same bits.
template <typename T>
__global__ __launch_bounds__(256) void smooth_blend_kernel(const T *__restrict__ pred, const double *__restrict__ win, SmoothGeom gm,
                                                           double *__restrict__ out)
{
    const int xo = blockIdx.x * 16 + (threadIdx.x & 15);
    const int yo = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (xo >= gm.ww || yo >= gm.hh) return;
    const int y = yo + gm.aug, x = xo + gm.aug;
    const double div = (double)(gm.sub * gm.sub);
    double total = 0.0;
#pragma unroll
    for (int g = 0; g < 8; g++) {
        int u, v;
        smooth_pad_to_frame(g, y, x, gm.Hp, gm.Wp, u, v);
        const int na = gm.na[g & 1], nb = gm.nb[g & 1];
        // the tiles a with a step <= u < a step + ws (0 <= p = u - a step < ws for each of them); none in the uncovered strip
        int a_hi = u / gm.step; if (a_hi > na - 1) a_hi = na - 1;
        int a_lo = u - gm.ws + gm.step; a_lo = a_lo > 0 ? a_lo / gm.step : 0;
        int b_hi = v / gm.step; if (b_hi > nb - 1) b_hi = nb - 1;
        int b_lo = v - gm.ws + gm.step; b_lo = b_lo > 0 ? b_lo / gm.step : 0;
        double acc = 0.0;
        for (int a = a_lo; a <= a_hi; a++) {
            const int p = u - a * gm.step;
            for (int b = b_lo; b <= b_hi; b++) {
                const int q = v - b * gm.step;
                const T pv = pred[((size_t)(gm.tile_off[g] + a * nb + b) * gm.ws + p) * gm.ws + q];
                const double w2 = win[p] * win[q];
                acc = acc + (double)pv * w2;
            }
        }
        acc = acc / div;
        total = g == 0 ? acc : total + acc;
    }
    out[(size_t)yo * gm.ww + xo] = total / 8.0;
}
void launch_smooth_blend(const void *pred, bool pred_f64, const double *win1d, const SmoothGeom &g, double *out, hipStream_t s)
{
    const dim3 grid((g.ww + 15) / 16, (g.hh + 15) / 16);        // smooth_geom keeps the sides <= 2^19: at most 2^15 blocks a side
    if (pred_f64) hipLaunchKernelGGL(smooth_blend_kernel<double>, grid, dim3(256), 0, s, (const double *)pred, win1d, g, out);
    else hipLaunchKernelGGL(smooth_blend_kernel<float>, grid, dim3(256), 0, s, (const float *)pred, win1d, g, out);
}

__global__ void widen_f32_kernel(const float *__restrict__ in, double *__restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = (double)in[i];
}
void launch_widen_f32(const float *in, double *out, size_t n, hipStream_t s)
{
    const size_t b = (n + 255) / 256;
    hipLaunchKernelGGL(widen_f32_kernel, dim3((unsigned)(b < 8192 ? (b ? b : 1) : 8192)), dim3(256), 0, s, in, out, n);
}

// device time between the session's two events, after the stream has drained; 0 when they were never recorded
static double smooth_elapsed_ms(SmoothSession &ss)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, ss.ev[0], ss.ev[1]) == hipSuccess ? (double)ms : 0.0;
}

}  // namespace tmat

using namespace tmat;

extern "C" {

int tmat_smooth_plan(int hh, int ww, int window_size, int subdivisions, int *aug, int *step, int counts[4], int *n_tiles)
{
    SmoothGeom g;
    if (!smooth_geom(hh, ww, window_size, subdivisions, g)) return TMAT_E_ARG;
    if (aug) *aug = g.aug;
    if (step) *step = g.step;
    if (counts) { counts[0] = g.na[0]; counts[1] = g.nb[0]; counts[2] = g.na[1]; counts[3] = g.nb[1]; }
    if (n_tiles) *n_tiles = g.n_tiles;
    return TMAT_OK;
}

int tmat_spline_window(int window_size, double *win)
{
    if (window_size < 4 || window_size > (1 << 15) || !win) { set_error("tmat_spline_window: needs window_size >= 4 and an output array"); return TMAT_E_ARG; }
    const std::vector<double> w = spline_window_host(window_size);
    std::copy(w.begin(), w.end(), win);
    return TMAT_OK;
}

int tmat_smooth_begin(tmat_handle h, const float *x, int hh, int ww, int window_size, int subdivisions, int *n_tiles)
{
    Ctx *c = (Ctx *)h;
    if (!c || !x) { set_error("tmat_smooth_begin: bad argument"); return TMAT_E_ARG; }
    SmoothGeom g;
    if (!smooth_geom(hh, ww, window_size, subdivisions, g)) return TMAT_E_ARG;
    TMAT_HIP(hipSetDevice(c->device));
    SmoothSession &ss = c->smooth;
    TMAT_HIP(hipStreamSynchronize(c->stream));
    ss.close();                                 // a second begin discards an open session
    for (hipEvent_t &e : ss.ev) if (!e) TMAT_HIP(hipEventCreate(&e));
    ss.g = g;
    ss.tiles_ms = ss.blend_ms = 0;
    const size_t per = (size_t)hh * ww;
    ss.x = (float *)ss.mem.dev(per * sizeof(float), "hipMalloc(smooth image)");
    ss.padval = (float *)ss.mem.dev(2 * sizeof(float), "hipMalloc(smooth pad value)");
    ss.win = (double *)ss.mem.dev((size_t)g.ws * sizeof(double), "hipMalloc(smooth window)");
    if (!ss.x || !ss.padval || !ss.win) { ss.close(); return TMAT_E_HIP; }
    DevScope mem(c->ws_pool, c->stream);
    mem.h2d(ss.x, x, per * sizeof(float));
    mem.h2d(ss.win, mem.keep(spline_window_host(g.ws)), (size_t)g.ws * sizeof(double));
    launch_minmax_f32(ss.x, 1, per, ss.padval, ss.padval + 1, c->stream);       // the pad value: img.min() (:77)
    mem.check(hipGetLastError(), "smooth_begin launch");
    if (mem.finish()) { ss.close(); return TMAT_E_HIP; }
    ss.have.assign(g.n_tiles, 0);
    ss.open = true;
    if (n_tiles) *n_tiles = g.n_tiles;
    return TMAT_OK;
}

static bool smooth_range_ok(const Ctx *c, int first, int count, const void *p, const char *who)
{
    if (!c || !p) { set_error(std::string(who) + ": bad argument"); return false; }
    if (!c->smooth.open) { set_error(std::string(who) + ": no open session (tmat_smooth_begin)"); return false; }
    if (first < 0 || count < 0 || first > c->smooth.g.n_tiles || count > c->smooth.g.n_tiles - first) {
        set_error(std::string(who) + ": tile range outside [0, n_tiles)");
        return false;
    }
    return true;
}

int tmat_smooth_tiles(tmat_handle h, int first, int count, float *patches)
{
    Ctx *c = (Ctx *)h;
    if (!smooth_range_ok(c, first, count, patches, "tmat_smooth_tiles")) return TMAT_E_ARG;
    if (count == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    SmoothSession &ss = c->smooth;
    const size_t n = (size_t)count * ss.g.ws * ss.g.ws;
    DevScope mem(c->ws_pool, c->stream);
    float *pd = mem.pooled<float>(n);
    if (!mem.ok) return TMAT_E_HIP;
    mem.check(hipEventRecord(ss.ev[0], c->stream), "hipEventRecord");
    launch_smooth_tiles(ss.x, ss.padval, ss.g, first, count, pd, c->stream);
    mem.check(hipGetLastError(), "smooth_tiles launch");
    mem.check(hipEventRecord(ss.ev[1], c->stream), "hipEventRecord");
    mem.d2h(patches, pd, n * sizeof(float));
    if (mem.finish()) return TMAT_E_HIP;
    ss.tiles_ms += smooth_elapsed_ms(ss);
    return TMAT_OK;
}

int tmat_smooth_put(tmat_handle h, int first, int count, const void *preds, int dtype)
{
    Ctx *c = (Ctx *)h;
    if (!smooth_range_ok(c, first, count, preds, "tmat_smooth_put")) return TMAT_E_ARG;
    if (dtype != TMAT_SMOOTH_F32 && dtype != TMAT_SMOOTH_F64) { set_error("tmat_smooth_put: dtype must be TMAT_SMOOTH_F32 or TMAT_SMOOTH_F64"); return TMAT_E_ARG; }
    SmoothSession &ss = c->smooth;
    const bool f64 = dtype == TMAT_SMOOTH_F64;
    if (ss.pred && ss.pred_f64 && !f64) { set_error("tmat_smooth_put: this session holds float64 predictions; widen float32 ones before the call"); return TMAT_E_ARG; }
    if (count == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t pp = (size_t)ss.g.ws * ss.g.ws, all = pp * ss.g.n_tiles;
    DevScope mem(c->ws_pool, c->stream);
    if (!ss.pred) {
        ss.pred = ss.mem.dev(all * (f64 ? sizeof(double) : sizeof(float)), "hipMalloc(smooth predictions)");
        if (!ss.pred) return TMAT_E_HIP;
        ss.pred_f64 = f64;
    } else if (f64 && !ss.pred_f64) {
        // the predictor went from float32 to float64: widen what is stored.  No bit of the result changes, the blend widens before
        // its first multiplication
        double *wide = (double *)ss.mem.dev(all * sizeof(double), "hipMalloc(smooth predictions, f64)");
        if (!wide) return TMAT_E_HIP;
        launch_widen_f32((const float *)ss.pred, wide, all, c->stream);
        if (!mem.check(hipGetLastError(), "widen launch") || mem.finish()) { ss.mem.release(wide); return TMAT_E_HIP; }
        ss.mem.release(ss.pred);
        ss.pred = wide;
        ss.pred_f64 = true;
    }
    const size_t el = ss.pred_f64 ? sizeof(double) : sizeof(float);
    mem.h2d((char *)ss.pred + (size_t)first * pp * el, preds, (size_t)count * pp * el);
    if (mem.finish()) return TMAT_E_HIP;
    std::fill(ss.have.begin() + first, ss.have.begin() + first + count, (uint8_t)1);
    return TMAT_OK;
}

int tmat_smooth_end(tmat_handle h, double *out)
{
    Ctx *c = (Ctx *)h;
    if (!c || !out) { set_error("tmat_smooth_end: bad argument"); return TMAT_E_ARG; }
    SmoothSession &ss = c->smooth;
    if (!ss.open) { set_error("tmat_smooth_end: no open session (tmat_smooth_begin)"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t missing = std::count(ss.have.begin(), ss.have.end(), (uint8_t)0);
    if (missing) {      // the session stays open: the caller may put the rest, or begin again
        set_error("tmat_smooth_end: " + std::to_string(missing) + " of " + std::to_string(ss.g.n_tiles) + " tiles were never put");
        return TMAT_E_ARG;
    }
    int rc;
    {
        const size_t per = (size_t)ss.g.hh * ss.g.ww;
        DevScope mem(c->ws_pool, c->stream);
        double *od = mem.pooled<double>(per);
        if (mem.ok) {
            mem.check(hipEventRecord(ss.ev[0], c->stream), "hipEventRecord");
            launch_smooth_blend(ss.pred, ss.pred_f64, ss.win, ss.g, od, c->stream);
            mem.check(hipGetLastError(), "smooth_blend launch");
            mem.check(hipEventRecord(ss.ev[1], c->stream), "hipEventRecord");
            mem.d2h(out, od, per * sizeof(double));
        }
        rc = mem.finish();
        if (!rc) ss.blend_ms = smooth_elapsed_ms(ss);
    }
    ss.close();
    return rc;
}

int tmat_debug_smooth_times(tmat_handle h, double *tiles_ms, double *blend_ms)
{
    Ctx *c = (Ctx *)h;
    if (!c || !tiles_ms || !blend_ms) { set_error("tmat_debug_smooth_times: bad argument"); return TMAT_E_ARG; }
    *tiles_ms = c->smooth.tiles_ms;
    *blend_ms = c->smooth.blend_ms;
    return TMAT_OK;
}

int tmat_predict_smooth_ex(tmat_handle h, const float *x, int n, int hh, int ww, int subdivisions, double *pred)
{
    if (subdivisions == 2) return tmat_predict_smooth(h, x, n, hh, ww, pred);       // the same code path, launches and region forms
    Ctx *c = (Ctx *)h;
    if (c && !has_model(c)) { set_error("tmat_predict_smooth_ex: this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (!c || !x || !pred || n < 0) { set_error("tmat_predict_smooth_ex: bad argument"); return TMAT_E_ARG; }
    SmoothGeom g;
    if (!smooth_geom(hh, ww, c->patch, subdivisions, g)) return TMAT_E_ARG;
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t per = (size_t)hh * ww, pp = (size_t)g.ws * g.ws;
    DevScope mem(c->ws_pool, c->stream);
    float *xd = mem.alloc_from(x, n * per);
    double *pd = mem.alloc<double>(n * per, "hipMalloc(pred)");
    float *pv = mem.alloc<float>(2, "hipMalloc(pad value)");
    float *tiles = mem.alloc<float>(pp * g.n_tiles, "hipMalloc(tile predictions)");
    if (!mem.ok) return TMAT_E_HIP;
    if (c->norm_on) launch_norm_f32(xd, n * per, c->norm_mean, c->norm_std, c->stream);
    // the network full-frame, in chunks of what the activation workspace holds (patch_in has room for max_patches patches at least); the
    // region planners know subdivisions = 2 only
    for (int i = 0; i < n; i++) {
        const float *xi = xd + (size_t)i * per;
        launch_minmax_f32(xi, 1, per, pv, pv + 1, c->stream);
        for (int t0 = 0; t0 < g.n_tiles; t0 += c->max_patches) {
            const int k = std::min(c->max_patches, g.n_tiles - t0);
            launch_smooth_tiles(xi, pv, g, t0, k, c->patch_in, c->stream);
            const int rc = unet_forward_dev(c, c->patch_in, k, tiles + (size_t)t0 * pp, c->stream);
            if (rc) return rc;
        }
        launch_smooth_blend(tiles, false, c->win1d, g, pd + (size_t)i * per, c->stream);
    }
    mem.check(hipGetLastError(), "predict_smooth_ex launch");
    mem.d2h(pred, pd, n * per * sizeof(double));
    return mem.finish();
}

}  // extern "C"
