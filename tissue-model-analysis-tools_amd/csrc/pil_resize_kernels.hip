// Pillow's resize of a mode-"F" (float32) image, LANCZOS and NEAREST, and UNetXceptionPatchSegmentor.predict(x, auto_resample=True)
// (reference models.py:624-653) as one device chain around the smooth prediction.
//
// LANCZOS is Pillow's two-pass convolution resample.  Per axis: scale = in / out, fs = max(scale, 1), support = 3 fs; for output index
// xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) - xmin, taps
// k[x] = L((x + xmin - center + 0.5) / fs) with L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3 (sinc by libm's sin, in f64), divided by
// their sequential sum.  The horizontal pass runs first; an output is an f64 sum from 0.0 over ascending taps of (double)pixel * k[x],
// stored as f32; the vertical pass reads that f32 image.  A pass whose sizes are equal is skipped.
// NEAREST is Pillow's affine scale: per axis a0 = in / out, xo = 0.5 a0, the source index of each output index in turn is (int)xo,
// then xo += a0 (the sum accumulates).
// The tap and index tables are made on the host (tmat_host_resize_pil_f32 uses the same ones) and uploaded; one thread per output pixel.
#include "tmat_ctx.h"

#include <cmath>

namespace tmat {

struct PilTaps {
    int ksize = 0;
    std::vector<int> bounds;        // [out][2]: xmin, count
    std::vector<double> kk;         // [out][ksize]
};

static double pil_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
static double pil_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? pil_sinc(x) * pil_sinc(x / 3) : 0.0; }

static PilTaps pil_lanczos_taps(int in, int out)
{
    PilTaps t;
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs;
    t.ksize = (int)std::ceil(support) * 2 + 1;
    t.bounds.assign((size_t)out * 2, 0);
    t.kk.assign((size_t)out * t.ksize, 0.0);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double *k = &t.kk[(size_t)xx * t.ksize];
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) {
            const double w = pil_lanczos((x + xmin - center + 0.5) / fs);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; x++) if (ww != 0.0) k[x] /= ww;
        t.bounds[2 * xx] = xmin;
        t.bounds[2 * xx + 1] = xmax;
    }
    return t;
}

// source index per output index; -1: outside the image (Pillow leaves such a pixel 0)
static std::vector<int> pil_nearest_index(int in, int out)
{
    std::vector<int> idx(out);
    const double a0 = (double)in / out;
    double xo = 0.5 * a0;
    for (int i = 0; i < out; i++) {
        const int xin = xo < 0.0 ? -1 : (int)xo;
        idx[i] = xin < in ? xin : -1;
        xo += a0;
    }
    return idx;
}

static bool pil_args_ok(const void *x, int n, int H, int W, int oh, int ow, int filter, const void *out, const char *who)
{
    const int lim = 1 << 15;
    if (!x || !out || n < 0 || H < 1 || W < 1 || oh < 1 || ow < 1 || H > lim || W > lim || oh > lim || ow > lim ||
        (filter != TMAT_PIL_NEAREST && filter != TMAT_PIL_LANCZOS) ||
        (long long)n * std::max(H, oh) * std::max(W, ow) > (1LL << 31) - 1) {
        set_error(std::string(who) + ": bad argument (sizes 1 .. 32768, fewer than 2^31 pixels, filter TMAT_PIL_NEAREST or TMAT_PIL_LANCZOS)");
        return false;
    }
    return true;
}

// ---- host twin ----
static void pil_lanczos_host(const float *x, int H, int W, int oh, int ow, float *out)
{
    std::vector<float> tmp;
    const float *src = x;
    if (ow != W) {
        const PilTaps t = pil_lanczos_taps(W, ow);
        float *dst = oh != H ? (tmp.resize((size_t)H * ow), tmp.data()) : out;
        for (int y = 0; y < H; y++)
            for (int xx = 0; xx < ow; xx++) {
                const int x0 = t.bounds[2 * xx], cnt = t.bounds[2 * xx + 1];
                const double *k = &t.kk[(size_t)xx * t.ksize];
                double ss = 0.0;
                for (int i = 0; i < cnt; i++) ss += (double)x[(size_t)y * W + x0 + i] * k[i];
                dst[(size_t)y * ow + xx] = (float)ss;
            }
        src = dst;
    }
    if (oh != H) {
        const PilTaps t = pil_lanczos_taps(H, oh);
        for (int yy = 0; yy < oh; yy++) {
            const int y0 = t.bounds[2 * yy], cnt = t.bounds[2 * yy + 1];
            const double *k = &t.kk[(size_t)yy * t.ksize];
            for (int xx = 0; xx < ow; xx++) {
                double ss = 0.0;
                for (int i = 0; i < cnt; i++) ss += (double)src[(size_t)(y0 + i) * ow + xx] * k[i];
                out[(size_t)yy * ow + xx] = (float)ss;
            }
        }
    }
    if (ow == W && oh == H) std::copy(x, x + (size_t)H * W, out);
}

// ---- device ----
// in (n, H, W) -> out (n, H, ow)
__global__ __launch_bounds__(256) void pil_resample_h_kernel(const float *__restrict__ in, size_t total, int W, int ow, const int *__restrict__ bounds,
                                                             const double *__restrict__ kk, int ksize, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / ow;
    const int xx = (int)(i - row * ow);
    const int x0 = bounds[2 * xx], cnt = bounds[2 * xx + 1];
    const float *p = in + row * W + x0;
    const double *k = kk + (size_t)xx * ksize;
    double ss = 0.0;
    for (int t = 0; t < cnt; t++) ss += (double)p[t] * k[t];
    out[i] = (float)ss;
}
// in (n, H, W) -> out (n, oh, W)
__global__ __launch_bounds__(256) void pil_resample_v_kernel(const float *__restrict__ in, size_t total, int H, int W, int oh, const int *__restrict__ bounds,
                                                             const double *__restrict__ kk, int ksize, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / W;
    const int xx = (int)(i - row * W);
    const size_t img = row / oh;
    const int yy = (int)(row - img * oh);
    const int y0 = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    const float *p = in + (img * H + y0) * W + xx;
    const double *k = kk + (size_t)yy * ksize;
    double ss = 0.0;
    for (int t = 0; t < cnt; t++) ss += (double)p[(size_t)t * W] * k[t];
    out[i] = (float)ss;
}
// in (n, H, W) -> out (n, oh, ow) through the index tables
__global__ __launch_bounds__(256) void pil_nearest_kernel(const float *__restrict__ in, size_t total, int H, int W, int oh, int ow, const int *__restrict__ yi,
                                                          const int *__restrict__ xi, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / ow;
    const int xx = (int)(i - row * ow);
    const size_t img = row / oh;
    const int yy = (int)(row - img * oh);
    const int sy = yi[yy], sx = xi[xx];
    out[i] = sy >= 0 && sx >= 0 ? in[(img * H + sy) * W + sx] : 0.f;
}
// Image.fromarray(float64 array): Pillow stores mode "F", a C cast to float
__global__ __launch_bounds__(256) void narrow_f64_kernel(const double *__restrict__ in, size_t total, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out[i] = (float)in[i];
}

static unsigned blocks_of(size_t total) { return (unsigned)((total + 255) / 256); }

// x_dev (n, H, W) -> out_dev (n, oh, ow), tables and the intermediate image from the scope; false when the scope failed
static bool pil_resize_dev(DevScope &mem, hipStream_t s, const float *x_dev, int n, int H, int W, int oh, int ow, int filter, float *out_dev)
{
    const size_t in_px = (size_t)n * H * W, out_px = (size_t)n * oh * ow;
    if (n == 0) return mem.ok;
    if (filter == TMAT_PIL_NEAREST) {
        const int *yi = mem.pooled_from(mem.keep(pil_nearest_index(H, oh)), (size_t)oh);
        const int *xi = mem.pooled_from(mem.keep(pil_nearest_index(W, ow)), (size_t)ow);
        if (!mem.ok) return false;
        hipLaunchKernelGGL(pil_nearest_kernel, dim3(blocks_of(out_px)), dim3(256), 0, s, x_dev, out_px, H, W, oh, ow, yi, xi, out_dev);
        return mem.check(hipGetLastError(), "pil_nearest launch");
    }
    if (ow == W && oh == H) return mem.check(hipMemcpyAsync(out_dev, x_dev, in_px * sizeof(float), hipMemcpyDeviceToDevice, s), "D2D");
    const float *src = x_dev;
    if (ow != W) {
        PilTaps t = pil_lanczos_taps(W, ow);
        const int ksize = t.ksize;
        const int *b = mem.pooled_from(mem.keep(std::move(t.bounds)), (size_t)ow * 2);
        const double *k = mem.pooled_from(mem.keep(std::move(t.kk)), (size_t)ow * ksize);
        float *dst = oh != H ? mem.pooled<float>((size_t)n * H * ow) : out_dev;
        if (!mem.ok) return false;
        hipLaunchKernelGGL(pil_resample_h_kernel, dim3(blocks_of((size_t)n * H * ow)), dim3(256), 0, s, x_dev, (size_t)n * H * ow, W, ow, b, k, ksize, dst);
        if (!mem.check(hipGetLastError(), "pil_resample_h launch")) return false;
        src = dst;
    }
    if (oh != H) {
        PilTaps t = pil_lanczos_taps(H, oh);
        const int ksize = t.ksize;
        const int *b = mem.pooled_from(mem.keep(std::move(t.bounds)), (size_t)oh * 2);
        const double *k = mem.pooled_from(mem.keep(std::move(t.kk)), (size_t)oh * ksize);
        if (!mem.ok) return false;
        hipLaunchKernelGGL(pil_resample_v_kernel, dim3(blocks_of(out_px)), dim3(256), 0, s, src, out_px, H, ow, oh, b, k, ksize, out_dev);
        if (!mem.check(hipGetLastError(), "pil_resample_v launch")) return false;
    }
    return mem.ok;
}

}  // namespace tmat

using namespace tmat;

extern "C" {

int tmat_host_resize_pil_f32(const float *x, int n, int H, int W, int out_h, int out_w, int filter, float *out)
{
    if (!pil_args_ok(x, n, H, W, out_h, out_w, filter, out, "tmat_host_resize_pil_f32")) return TMAT_E_ARG;
    std::vector<int> yi, xi;
    if (filter == TMAT_PIL_NEAREST) { yi = pil_nearest_index(H, out_h); xi = pil_nearest_index(W, out_w); }
    for (int i = 0; i < n; i++) {
        const float *src = x + (size_t)i * H * W;
        float *dst = out + (size_t)i * out_h * out_w;
        if (filter == TMAT_PIL_LANCZOS) { pil_lanczos_host(src, H, W, out_h, out_w, dst); continue; }
        for (int yy = 0; yy < out_h; yy++)
            for (int xx = 0; xx < out_w; xx++)
                dst[(size_t)yy * out_w + xx] = yi[yy] >= 0 && xi[xx] >= 0 ? src[(size_t)yi[yy] * W + xi[xx]] : 0.f;
    }
    return TMAT_OK;
}

int tmat_resize_pil_f32(tmat_handle h, const float *x, int n, int H, int W, int out_h, int out_w, int filter, float *out)
{
    Ctx *c = (Ctx *)h;
    if (!c) { set_error("tmat_resize_pil_f32: null handle"); return TMAT_E_ARG; }
    if (!pil_args_ok(x, n, H, W, out_h, out_w, filter, out, "tmat_resize_pil_f32")) return TMAT_E_ARG;
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    DevScope mem(c->ws_pool, c->stream);
    const float *xd = mem.pooled_from(x, (size_t)n * H * W);
    float *od = mem.pooled<float>((size_t)n * out_h * out_w);
    if (!mem.ok || !pil_resize_dev(mem, c->stream, xd, n, H, W, out_h, out_w, filter, od)) return TMAT_E_HIP;
    mem.d2h(out, od, (size_t)n * out_h * out_w * sizeof(float));
    return mem.finish();
}

int tmat_predict_auto_resample(tmat_handle h, const float *x, int H, int W, int mid_h, int mid_w, int out_h, int out_w, float *out)
{
    Ctx *c = (Ctx *)h;
    if (c && !has_model(c)) { set_error("tmat_predict_auto_resample: this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (!c) { set_error("tmat_predict_auto_resample: null handle"); return TMAT_E_ARG; }
    if (!pil_args_ok(x, 1, H, W, mid_h, mid_w, TMAT_PIL_LANCZOS, out, "tmat_predict_auto_resample") ||
        !pil_args_ok(x, 1, mid_h, mid_w, out_h, out_w, TMAT_PIL_NEAREST, out, "tmat_predict_auto_resample")) return TMAT_E_ARG;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t mid = (size_t)mid_h * mid_w, outn = (size_t)out_h * out_w;
    DevScope mem(c->ws_pool, c->stream);
    const float *xd = mem.pooled_from(x, (size_t)H * W);
    float *xs = mem.pooled<float>(mid);             // the resampled image, normalised in place by the smooth prediction
    double *pd = mem.pooled<double>(mid);
    float *pf = mem.pooled<float>(mid);
    float *od = mem.pooled<float>(outn);
    if (!mem.ok || !pil_resize_dev(mem, c->stream, xd, 1, H, W, mid_h, mid_w, TMAT_PIL_LANCZOS, xs)) return TMAT_E_HIP;
    { const int rc = predict_smooth_dev(c, xs, 1, mid_h, mid_w, pd); if (rc) return rc; }
    hipLaunchKernelGGL(narrow_f64_kernel, dim3(blocks_of(mid)), dim3(256), 0, c->stream, pd, mid, pf);
    if (!mem.check(hipGetLastError(), "narrow launch") || !pil_resize_dev(mem, c->stream, pf, 1, mid_h, mid_w, out_h, out_w, TMAT_PIL_NEAREST, od)) return TMAT_E_HIP;
    mem.d2h(out, od, outn * sizeof(float));
    return mem.finish();
}

}  // extern "C"
