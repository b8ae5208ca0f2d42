// C-ABI entry points of libtmat_hip.so (see include/tmat.h) -- context, weights, UNet driver,
// smooth tiled prediction.  gfx950 only; there is deliberately no CPU fallback: every compute
// entry point needs a HIP device and fails loudly without one.
#include "../../include/tmat.h"
#include "tmat_ctx.h"
#include "png.h"
#include "tiff.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

namespace tmat {

// One process-wide message (the last error of any thread): entry points run stages on worker threads, and a message
// recorded there must reach the thread that called the entry point.
static std::mutex g_err_mu;
static std::string g_err;
void set_error(const std::string &msg)
{
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = msg;
}
bool hip_ok(hipError_t e, const char *what)
{
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

// ---------------------------------------------------------------------------------------------
// weight container ("TMATW001", tmat_amd/synth.py:pack_weights)
// ---------------------------------------------------------------------------------------------

bool parse_blob(const void *blob, size_t nbytes, std::map<std::string, Tensor> &out, int &patch)
{
    const uint8_t *p = (const uint8_t *)blob;
    if (nbytes < 16 || memcmp(p, "TMATW001", 8)) { set_error("weights: bad magic"); return false; }
    uint32_t n, ps;
    memcpy(&n, p + 8, 4); memcpy(&ps, p + 12, 4);
    patch = (int)ps;
    size_t pos = 16;
    for (uint32_t i = 0; i < n; i++, pos += 84) {
        if (pos + 84 > nbytes) { set_error("weights: truncated table"); return false; }
        char name[49]; memcpy(name, p + pos, 48); name[48] = 0;
        uint32_t ndim, d[4]; uint64_t off, cnt;
        memcpy(&ndim, p + pos + 48, 4); memcpy(d, p + pos + 52, 16);
        memcpy(&off, p + pos + 68, 8); memcpy(&cnt, p + pos + 76, 8);
        // overflow-safe bounds: off inside the blob, cnt floats fit behind it (no off + cnt * 4 that could wrap)
        if (ndim > 4 || off % 4 || off > nbytes || cnt > (nbytes - off) / 4) { set_error("weights: bad entry"); return false; }
        Tensor t; t.data = (const float *)(p + off); t.count = cnt;
        uint64_t prod = 1;
        for (uint32_t k = 0; k < ndim; k++) {
            if (d[k] == 0 || d[k] > (1u << 24) || prod > (1ull << 40)) { set_error("weights: bad dimension"); return false; }
            t.shape.push_back((int)d[k]); prod *= d[k];
        }
        if (prod != cnt) { set_error("weights: shape/count mismatch"); return false; }
        out[name] = t;
    }
    return true;
}

static bool upload(Ctx *c, const std::vector<float> &v, float **dev)
{
    if (!hip_ok(hipMalloc((void **)dev, v.size() * sizeof(float)), "hipMalloc(weights)")) return false;
    c->owned.push_back(*dev);
    return hip_ok(hipMemcpy(*dev, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(weights)");
}
// weights of an MFMA convolution ([taps][Cout][Cin], k contiguous): the host copy is kept so that tmat_set_precision can
// make the split-precision copy later
static bool upload_conv(Ctx *c, const std::vector<float> &v, int cin, float **dev)
{
    if (!upload(c, v, dev)) return false;
    c->conv_w_host[*dev] = ConvWHost{v, cin};
    return true;
}

// round-to-nearest-even f32 -> bf16 (finite inputs: weights)
static uint16_t bf16_rne(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_to_f32(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float x;
    memcpy(&x, &u, 4);
    return x;
}
// Split-precision copy of conv weights for conv_mfma_kernel<..., PREC = 1 | 2> (unet_kernels.hip): npl bf16 planes of the
// tensor's own layout, plane 0 = rne(w), plane 1 = rne(w - p0), plane 2 = rne(w - p0 - p1) (each difference is exact in f32).
// Returned as a float vector used as a byte container (npl * w.size() bf16 values).
static std::vector<float> split_bf16(const std::vector<float> &w, int npl)
{
    std::vector<float> out((w.size() * npl + 1) / 2);
    uint16_t *o = reinterpret_cast<uint16_t *>(out.data());
    const size_t n = w.size();
    for (size_t i = 0; i < n; i++) {
        float rem = w[i];
        for (int pl = 0; pl < npl; pl++) {
            const uint16_t q = bf16_rne(rem);
            o[(size_t)pl * n + i] = q;
            rem = rem - bf16_to_f32(q);
        }
    }
    return out;
}

// scale = f32(gamma / sqrt(var + eps)); shift = f32(beta + (bias - mean) * scale_f64)   (BN folding)
static void fold_bn(const Tensor &bn, const Tensor &bias, std::vector<float> &scale, std::vector<float> &shift)
{
    int C = bn.shape[1];
    scale.resize(C); shift.resize(C);
    for (int i = 0; i < C; i++) {
        double g = bn.data[i], b = bn.data[C + i], m = bn.data[2 * C + i], v = bn.data[3 * C + i];
        double sd = g / std::sqrt(v + 1e-3);
        scale[i] = (float)sd;
        shift[i] = (float)(b + ((double)bias.data[i] - m) * sd);
    }
}

// Keras Conv2DTranspose kernel (kh, kw, out, in), stride 1, SAME -> conv taps
// Wc[a][b][in][out] = K[2-a][2-b][out][in]
static std::vector<float> convt_as_conv(const Tensor &k)
{
    int O = k.shape[2], I = k.shape[3];
    std::vector<float> w((size_t)9 * I * O);
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            for (int i = 0; i < I; i++)
                for (int o = 0; o < O; o++)
                    w[(((size_t)a * 3 + b) * I + i) * O + o] = k.data[(((size_t)(2 - a) * 3 + (2 - b)) * O + o) * I + i];
    return w;
}

// Sub-pixel form of a 3x3 convolution over a 2x nearest-upsampled tensor (unet_kernels.hip, KS == 2): per output
// parity class (py, px) the taps that land on the same stored pixel are summed -- f32 adds from +0.0 in (ky, kx)
// order, as oracle/unet.py:subpixel_weights does.  [9][I][O] -> [4 classes][4 slots][I][O]
static std::vector<float> subpixel_weights(const std::vector<float> &w9, int I, int O)
{
    const size_t IO = (size_t)I * O;
    std::vector<float> w(16 * IO, 0.0f);
    for (int py = 0; py < 2; py++)
        for (int px = 0; px < 2; px++)
            for (int ky = 0; ky < 3; ky++)
                for (int kx = 0; kx < 3; kx++) {
                    const int a = ((py + ky - 1) >> 1) - (py - 1), b = ((px + kx - 1) >> 1) - (px - 1);
                    float *d = &w[((size_t)(py * 2 + px) * 4 + a * 2 + b) * IO];
                    const float *s = &w9[(size_t)(ky * 3 + kx) * IO];
                    for (size_t i = 0; i < IO; i++) d[i] = d[i] + s[i];
                }
    return w;
}

// [taps][I][O] -> [taps][O][I]: the MFMA convolution reads both operands k-contiguous (unet_kernels.hip)
std::vector<float> k_contiguous(const float *w, int taps, int I, int O)
{
    std::vector<float> r((size_t)taps * I * O);
    for (int t = 0; t < taps; t++)
        for (int i = 0; i < I; i++)
            for (int o = 0; o < O; o++) r[((size_t)t * O + o) * I + i] = w[((size_t)t * I + i) * O + o];
    return r;
}

static bool need(const std::map<std::string, Tensor> &m, const std::string &k, Tensor &t)
{
    auto it = m.find(k);
    if (it == m.end()) { set_error("weights: missing tensor " + k); return false; }
    t = it->second;
    return true;
}
// shape checks of what build_model indexes: a BatchNormalization block is (4, C) [gamma, beta, mean, var], a bias is (C)
static bool bn_ok(const Tensor &bn, const Tensor &bias, int C)
{
    if (bn.shape.size() != 2 || bn.shape[0] != 4 || bn.shape[1] != C || (int)bias.count != C) {
        set_error("weights: BatchNormalization / bias tensor does not match its convolution");
        return false;
    }
    return true;
}

static bool build_model(Ctx *c, const std::map<std::string, Tensor> &m)
{
    Tensor w, b, bn;
    std::vector<float> sc, sh;
    if (!need(m, "stem.w", w) || !need(m, "stem.b", b) || !need(m, "stem.bn", bn)) return false;
    if (w.shape.size() != 4 || w.shape[2] != 1) { set_error("weights: only channels=1 supported"); return false; }
    c->f0 = w.shape[3];
    if (w.shape[0] != 3 || w.shape[1] != 3) { set_error("weights: stem must be 3x3"); return false; }
    if (!bn_ok(bn, b, c->f0)) return false;
    fold_bn(bn, b, sc, sh);
    if (!upload(c, std::vector<float>(w.data, w.data + w.count), &c->stem_w) || !upload(c, sc, &c->stem_scale) ||
        !upload(c, sh, &c->stem_shift)) return false;
    int cin = c->f0;
    for (int i = 0;; i++) {
        std::string p = "down" + std::to_string(i);
        if (!m.count(p + ".sep1.dw")) break;
        DownBlock d; d.cin = cin;
        Tensor dw, pw, rb;
        for (int s = 0; s < 2; s++) {
            std::string sp = p + (s ? ".sep2" : ".sep1");
            if (!need(m, sp + ".dw", dw) || !need(m, sp + ".pw", pw) || !need(m, sp + ".b", b) ||
                !need(m, p + (s ? ".bn2" : ".bn1"), bn)) return false;
            if (dw.shape.size() != 3 || pw.shape.size() != 2 || dw.count != (size_t)9 * pw.shape[0] || pw.shape[0] != (s ? d.cout : d.cin) ||
                !bn_ok(bn, b, pw.shape[1])) {
                set_error("weights: separable convolution tensors of " + sp + " have unexpected shapes");
                return false;
            }
            fold_bn(bn, b, sc, sh);
            if (!upload(c, std::vector<float>(dw.data, dw.data + dw.count), &d.dw[s]) ||
                !upload_conv(c, k_contiguous(pw.data, 1, pw.shape[0], pw.shape[1]), pw.shape[0], &d.pw[s]) || !upload(c, sc, &d.scale[s]) ||
                !upload(c, sh, &d.shift[s])) return false;
            d.cout = pw.shape[1];
        }
        if (!need(m, p + ".res.w", w) || !need(m, p + ".res.b", rb)) return false;
        if (w.count != (size_t)d.cin * d.cout || (int)rb.count != d.cout) { set_error("weights: residual convolution of " + p + " has unexpected shape"); return false; }
        if (!upload_conv(c, k_contiguous(w.data, 1, d.cin, d.cout), d.cin, &d.res_w) ||
            !upload(c, std::vector<float>(rb.data, rb.data + rb.count), &d.res_b)) return false;
        c->down.push_back(d);
        cin = d.cout;
    }
    for (int j = 0;; j++) {
        std::string p = "up" + std::to_string(j);
        if (!m.count(p + ".ct1.w")) break;
        UpBlock u; u.cin = cin;
        Tensor rb;
        for (int s = 0; s < 2; s++) {
            std::string sp = p + (s ? ".ct2" : ".ct1");
            if (!need(m, sp + ".w", w) || !need(m, sp + ".b", b) || !need(m, p + (s ? ".bn2" : ".bn1"), bn)) return false;
            if (w.shape.size() != 4 || w.shape[0] != 3 || w.shape[1] != 3) { set_error("weights: ConvT must be 3x3"); return false; }
            if (w.shape[3] != (s ? w.shape[2] : u.cin) || !bn_ok(bn, b, w.shape[2])) { set_error("weights: transposed convolution tensors of " + sp + " have unexpected shapes"); return false; }
            fold_bn(bn, b, sc, sh);
            const std::vector<float> w9 = convt_as_conv(w);
            const int I = w.shape[3], O = w.shape[2];
            if (!upload_conv(c, k_contiguous(w9.data(), 9, I, O), I, &u.ct[s]) || !upload(c, sc, &u.scale[s]) || !upload(c, sh, &u.shift[s])) return false;
            // blocks after the first read a 2x nearest-upsampled tensor in their first convolution: sub-pixel form
            if (s == 0 && j > 0 && !upload_conv(c, k_contiguous(subpixel_weights(w9, I, O).data(), 16, I, O), I, &u.ct_sub)) return false;
            u.cout = w.shape[2];
        }
        if (!need(m, p + ".res.w", w) || !need(m, p + ".res.b", rb)) return false;
        if (w.count != (size_t)u.cin * u.cout || (int)rb.count != u.cout) { set_error("weights: residual convolution of " + p + " has unexpected shape"); return false; }
        if (!upload_conv(c, k_contiguous(w.data, 1, u.cin, u.cout), u.cin, &u.res_w) ||
            !upload(c, std::vector<float>(rb.data, rb.data + rb.count), &u.res_b)) return false;
        c->up.push_back(u);
        cin = u.cout;
    }
    if (!need(m, "final.w", w) || !need(m, "final.b", b)) return false;
    {   // final 3x3 conv over the upsampled tensor: sub-pixel form, laid out [C/4][class][slot][4] for unet_kernels.hip:final_kernel
        const int C = cin;
        if ((int)w.count != 9 * C || C % 4) { set_error("weights: final conv must be 3x3xCx1"); return false; }
        const std::vector<float> sub = subpixel_weights(std::vector<float>(w.data, w.data + w.count), C, 1);   // [4][4][C]
        std::vector<float> q((size_t)16 * C);
        for (int cg = 0; cg < C / 4; cg++)
            for (int ct = 0; ct < 16; ct++)
                for (int e = 0; e < 4; e++) q[((size_t)cg * 16 + ct) * 4 + e] = sub[(size_t)ct * C + cg * 4 + e];
        if (!upload(c, q, &c->final_w)) return false;
    }
    c->final_b = b.data[0];
    c->f_last = cin;
    if (c->down.size() != c->up.size() - 1 || c->down.empty()) { set_error("weights: unexpected block structure"); return false; }
    int P = c->patch;
    if (P % (8 << c->down.size()) || P <= 0) { set_error("weights: patch size must be divisible by 2^(blocks+1)"); return false; }
    return true;
}

// ---------------------------------------------------------------------------------------------
// What a blob's forward launches (host arithmetic only: tmat_model_layers, and tmat_create before it allocates anything)
// ---------------------------------------------------------------------------------------------
struct ModelShape {
    int patch = 0, f0 = 0;
    std::vector<std::pair<int, int>> down, up;      // (cin, cout) per block
};
struct ModelLayer { int ksize, stride, cin, cout, side, launcher; };

// the channel counts of the blob's blocks, from the tensors build_model reads them from
static bool model_shape(const std::map<std::string, Tensor> &m, int patch, ModelShape &ms)
{
    ms = ModelShape();
    ms.patch = patch;
    Tensor w;
    if (!need(m, "stem.w", w)) return false;
    if (w.shape.size() != 4 || w.shape[2] != 1) { set_error("weights: only channels=1 supported"); return false; }
    int cin = ms.f0 = w.shape[3];
    for (int i = 0;; i++) {
        const std::string p = "down" + std::to_string(i);
        if (!m.count(p + ".sep1.dw")) break;
        if (!need(m, p + ".sep1.pw", w)) return false;
        if (w.shape.size() != 2 || w.shape[0] != cin) { set_error("weights: separable convolution tensors of " + p + ".sep1 have unexpected shapes"); return false; }
        ms.down.push_back({cin, w.shape[1]});
        cin = w.shape[1];
    }
    for (int j = 0;; j++) {
        const std::string p = "up" + std::to_string(j);
        if (!m.count(p + ".ct1.w")) break;
        if (!need(m, p + ".ct1.w", w)) return false;
        if (w.shape.size() != 4 || w.shape[3] != cin) { set_error("weights: transposed convolution tensors of " + p + ".ct1 have unexpected shapes"); return false; }
        ms.up.push_back({cin, w.shape[2]});
        cin = w.shape[2];
    }
    if (ms.down.empty() || ms.up.size() != ms.down.size() + 1) { set_error("weights: unexpected block structure"); return false; }
    if (patch <= 0 || patch % (8 << ms.down.size())) { set_error("weights: patch size must be divisible by 2^(blocks+1)"); return false; }
    return true;
}

// does a down block at input side H run on the wave-specialised fused separable kernel?
static bool fused_level(bool fused_sep, int H, int cin, int cout)
{
    return fused_sep && sepconv_ws_supported(H, H, cin, cout) && sepconv_ws_supported(H, H, cout, cout) && ((cout / 4) & (cout / 4 - 1)) == 0;
}

// The switches of tmat_create that decide which kernel a layer runs on
struct UnetSwitches { bool fused_sep = true, stem_fused = true, fused_pool = true; };
static UnetSwitches unet_switches_from_env()
{
    UnetSwitches s;
    if (const char *e = getenv("TMAT_FUSED_SEP")) s.fused_sep = atoi(e) != 0;
    if (const char *e = getenv("TMAT_FUSED_POOL")) s.fused_pool = atoi(e) != 0;
    if (const char *e = getenv("TMAT_STEM_FUSED")) s.stem_fused = atoi(e) != 0;
    return s;
}

// Every convolution launch of one f32 forward (unet_down_dev, then unet_up_dev), in launch order: launcher 0 conv_mfma_kernel, 1 the
// narrow kernel (conv_narrow_kernels.hip), 2 the fused separable kernel; side: of the launch's output.  False with the rule in the
// error: a convolution neither launcher takes, or a channel count the down path's other kernels do not take.
static bool model_layers(const ModelShape &ms, const UnetSwitches &sw, std::vector<ModelLayer> &out)
{
    static const float mark = 0.f;          // a residual's presence is all the shape rules look at
    out.clear();
    auto pow2x4 = [](int C) { return C >= 4 && C % 4 == 0 && ((C / 4) & (C / 4 - 1)) == 0; };
    auto conv = [&](int ksize, int stride, int cin, int cout, int side_in, bool resid, int rs) {
        ConvArgs a{};
        a.N = 1; a.h = a.w = side_in; a.Cin = cin; a.ksize = ksize; a.stride = stride; a.Cout = cout; a.resid = resid ? &mark : nullptr; a.rs = rs;
        const int launcher = conv_mfma_takes(a) ? 0 : conv_narrow_takes(a) ? 1 : -1;
        if (launcher < 0) {
            set_error("weights: the convolution " + std::to_string(cin) + " -> " + std::to_string(cout) + " (ksize " + std::to_string(ksize) +
                      ") runs on neither convolution kernel: every filter count must be a multiple of 16, at least 16 (conv_mfma_kernel takes cin % 64 == 0, "
                      "% 32 in the sub-pixel form, and cout % 64 == 0; the narrow kernel cin % 16 == 0 and cout % 16 == 0)");
            return false;
        }
        out.push_back({ksize, stride, cin, cout, side_in / stride * (ksize == 2 ? 2 : 1), launcher});
        return true;
    };
    if (!pow2x4(ms.f0)) { set_error("weights: the stem's filter count must be 4 times a power of two"); return false; }
    int H = ms.patch / 2;
    for (size_t bi = 0; bi < ms.down.size(); bi++) {
        const int cin = ms.down[bi].first, cout = ms.down[bi].second;
        if (fused_level(sw.fused_sep, H, cin, cout)) {
            const bool stem_here = bi == 0 && sw.stem_fused && cin == ms.f0;        // the residual then reads the stem at the even pixels
            out.push_back({1, 1, cin, cout, H, 2});
            if (!conv(1, stem_here ? 1 : 2, cin, cout, stem_here ? H / 2 : H, false, 0)) return false;
            out.push_back({1, 1, cout, cout, sw.fused_pool ? H / 2 : H, 2});
        } else {
            // depthwise, pooling and pooling fix-up kernels index channel groups by shifts
            if (!pow2x4(cin) || !pow2x4(cout)) { set_error("weights: the filter counts of the down path must be 4 times a power of two"); return false; }
            if (!conv(1, 1, cin, cout, H, false, 0) || !conv(1, 1, cout, cout, H, false, 0) || !conv(1, 2, cin, cout, H, false, 0)) return false;
        }
        H /= 2;
    }
    int Hs = ms.patch >> (1 + ms.down.size()), up = 0;
    for (size_t j = 0; j < ms.up.size(); j++) {
        const int cin = ms.up[j].first, cout = ms.up[j].second;
        if (!conv(up ? 2 : 3, 1, cin, cout, Hs, false, 0) || !conv(1, 1, cin, cout, Hs, false, 0) || !conv(3, 1, cout, cout, Hs << up, true, up)) return false;
        Hs <<= up; up = 1;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// UNet forward on device patches X (n, P, P) -> Y (n, P, P); n <= max_patches.
// Buffer plan (4 ping-pong activation buffers) is documented in DESIGN.md.
// ---------------------------------------------------------------------------------------------
static void prof_begin(Ctx *c, double flops, hipStream_t st)
{
    if (!c->prof_on) return;
    hipEvent_t e0, e1;
    if (c->ev_pool.size() >= 2) { e0 = c->ev_pool.back(); c->ev_pool.pop_back(); e1 = c->ev_pool.back(); c->ev_pool.pop_back(); }
    else { hipEventCreate(&e0); hipEventCreate(&e1); }
    hipEventRecord(e0, st);
    c->ev_open.push_back({e0, e1, flops});
}
static void prof_end(Ctx *c, hipStream_t st)
{
    if (!c->prof_on) return;
    hipEventRecord(c->ev_open.back().e1, st);
}

static bool conv(Ctx *c, ConvArgs a, hipStream_t st, const RoiSegs *roi = nullptr)
{
    bool dom = a.ksize == 3 && a.Cout % 128 == 0 && !a.relu_in;     // the conv_mfma_kernel<128,128,4,2,3,false> instantiation
    if (dom) {      // the FLOPs the launch executes: region form -- its segments' pixels only
        const double px = roi ? (double)roi->pixels() : (double)a.N * a.h * a.w;
        prof_begin(c, 2.0 * px * 9.0 * a.Cin * a.Cout, st);
    }
    if (c->precision != TMAT_PRECISION_F32) {        // opt-in split precision: the same launch on the split copy of the weights
        auto &mp = c->wsplit[c->precision];
        auto it = mp.find(a.W);
        if (it != mp.end()) { a.W = it->second; a.prec = c->precision; }
    }
    // the narrow layers (16 / 32 channels: filter_counts below the shipped model's) run on the kernel of conv_narrow_kernels.hip; a
    // shape conv_mfma_kernel takes never does
    bool ok = conv_mfma_takes(a) ? launch_conv(a, st, roi) : launch_conv_narrow(a, st, roi);
    if (dom) prof_end(c, st);
    return ok;
}

// The tile table of fused separable layer `layer` for passes of k images under a form, cached on the plan's entry: built and uploaded on
// first use (a blocking copy into a fresh allocation, as for the patch order), never per pass.  dev stays null when every patch is
// computed whole.  Null + error set: the allocation or the copy failed.
// From ROI_DOWN_CONST upwards every tile of the k all-constant patches behind the pass's patches follows; the forms above
// ROI_DOWN_SHARE keep its table.
// quad: the quadrant table of the layer (roi_plan.h:roi_sep_quad_table for a plain layer 6 b + 1, roi_sep_quad_pool_table for a pooled
// layer 6 b + 3) where the plan has one for the form -- n packed tiles of four ids, the constant patches' quadrants and the padding
// included, always on the device; the tile table otherwise
static const RoiTileTab *roi_tile_tab(RoiEntry *e, int layer, int k, RoiDownForm form, bool quad = false)
{
    form = roi_down_form(e->plan, std::min(form, ROI_DOWN_SHARE));
    for (const RoiTileTab &t : e->tabs) if (t.layer == layer && t.k == k && t.form == form && t.quad == quad) return &t;
    std::vector<int> ids;
    RoiTileTab t;
    t.layer = layer; t.k = k; t.form = form;
    if (quad) {
        long long n_own = 0, n_ids = 0;
        t.full_rep = t.full = (layer % 6 == 3 ? roi_sep_quad_pool_table : roi_sep_quad_table)(e->plan, form, layer, k, ids, &n_own, &n_ids);
        if (t.full > 0) {
            t.quad = true;
            t.n = (int)(ids.size() / 4);
            t.n_rep = (n_own + 3) / 4;              // packed tiles of the pass's own patches
            if (!hip_ok(hipMalloc((void **)&t.dev, ids.size() * sizeof(int)), "hipMalloc(quadrant table)")) return nullptr;
            if (!hip_ok(hipMemcpy(t.dev, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(quadrant table)")) { hipFree(t.dev); return nullptr; }
            e->tabs.push_back(t);
            return &e->tabs.back();
        }
        return roi_tile_tab(e, layer, k, form);     // no quadrant table for this layer and form: the tile table
    }
    t.full = roi_sep_tile_table(e->plan, form, layer, k, ids);
    t.n_rep = (long long)ids.size(); t.full_rep = t.full;
    if (t.full <= 0 || ids.empty()) { set_error("roi_tile_tab: no tile table for this layer"); return nullptr; }
    if (form >= ROI_DOWN_CONST) {
        const int TW = e->plan.down.res[layer] / 16, TPP = TW * TW;
        if (t.full + (long long)k * TPP > 0x7fffffffLL) { set_error("roi_tile_tab: too many tiles"); return nullptr; }
        for (int id = (int)t.full; id < (int)t.full + k * TPP; id++) ids.push_back(id);
        t.full += (long long)k * TPP;
    }
    t.n = (int)ids.size();
    if ((long long)ids.size() < t.full) {
        if (!hip_ok(hipMalloc((void **)&t.dev, ids.size() * sizeof(int)), "hipMalloc(tile table)")) return nullptr;
        if (!hip_ok(hipMemcpy(t.dev, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(tile table)")) { hipFree(t.dev); return nullptr; }
    }
    e->tabs.push_back(t);
    return &e->tabs.back();
}

// The neighbour copies of passes of k images under a form (ROI_DOWN_SHARE or above), cached on the plan's entry like the tile tables:
// the neighbour table and, per stored tensor, the items the form copies (roi_plan.h:roi_down_copy_items), built and uploaded on first
// use, never per pass.  Null + error set: an allocation or a copy failed.
static const RoiShareTab *roi_share_tab(RoiEntry *e, int k, RoiDownForm form)
{
    for (const RoiShareTab &t : e->shares) if (t.k == k && t.form == form) return &t;
    const RoiPlan &p = e->plan;
    RoiShareTab t;
    t.k = k; t.form = form;
    roi_share_neighbours(p, k, t.nbr);
    for (int l = 0; l < p.down.n_layers; l++) {
        RoiShareTab::Layer sl;
        sl.layer = l;
        roi_down_copy_items(p, form, l, k, sl.items);
        if (!sl.items.empty()) t.layers.push_back(sl);
    }
    auto up = [](const void *src, size_t bytes, void **dev) {
        return bytes == 0 || (hip_ok(hipMalloc(dev, bytes), "hipMalloc(share table)") &&
                              hip_ok(hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice), "hipMemcpy(share table)"));
    };
    bool ok = up(t.nbr.data(), t.nbr.size() * sizeof(int), (void **)&t.nbr_dev);
    for (RoiShareTab::Layer &l : t.layers) ok = ok && up(l.items.data(), l.items.size() * sizeof(ShareItem), (void **)&l.dev);
    if (!ok) {
        if (t.nbr_dev) hipFree(t.nbr_dev);
        for (RoiShareTab::Layer &l : t.layers) if (l.dev) hipFree(l.dev);
        return nullptr;
    }
    e->shares.push_back(t);
    return &e->shares.back();
}

// does down block bi (input resolution P / 2 >> bi) run on the wave-specialised fused separable kernel?
static bool down_block_ws(const Ctx *c, size_t bi)
{
    const DownBlock &d = c->down[bi];
    const int H = (c->patch / 2) >> bi;
    return fused_level(c->fused_sep, H, d.cin, d.cout);
}

// the segments of a layer of the up path for a pass of k images: one per class with a non-empty rectangle, in the class-major patch
// order (of the set of up-path rectangles the handle launches: RoiPlan::up_rects)
static RoiSegs roi_segs(const RoiPlan &p, int l, int k)
{
    const RoiRect *rects = p.up_rects(l);
    RoiSegs r{};
    for (int cl = 0; cl < p.n_classes; cl++) {
        const RoiRect &q = rects[cl];
        if (q.rh <= 0 || q.rw <= 0 || p.class_count[cl] <= 0) continue;
        RoiSeg &g = r.s[r.nseg++];
        g.p0 = k * p.class_base[cl]; g.np = k * p.class_count[cl];
        g.y0 = q.y0; g.x0 = q.x0; g.rh = q.rh; g.rw = q.rw;
    }
    return r;
}

static RoiEntry *roi_entry_of(const Ctx *c, const RoiPlan *plan)
{
    for (RoiEntry *e : c->roi_cache) if (&e->plan == plan) return e;
    return nullptr;
}

RoiDownForm roi_down_resolve(const Ctx *c, const RoiPlan *plan, int kimg, bool have_padval, bool by_default)
{
    if (!plan || plan->n_classes <= 0 || plan->down.n_down != (int)c->down.size() || kimg < 1) return ROI_DOWN_FULL;
    auto on = [&](int sw) { return by_default ? sw != 0 : sw == 1; };
    RoiDownForm want = ROI_DOWN_REGION;
    // the constant-ring form: f32 path, some region form of the down path on, room for the constant patches and for their segment
    if (on(c->roi_const) && have_padval && c->roi_down && c->precision == TMAT_PRECISION_F32 && kimg <= c->const_cap &&
        plan->n_classes < ROI_MAX_CLASSES) want = ROI_DOWN_CONST;
    // the shared-interior form: with the constant-ring form and the tile tables (TMAT_ROI_DOWN bit 1) only
    if (want == ROI_DOWN_CONST && on(c->roi_share) && (c->roi_down & 2u) && roi_entry_of(c, plan)) want = ROI_DOWN_SHARE;
    // the rectangle launches' forms: where the shared-interior form runs and the rectangle launches are on (TMAT_ROI_DOWN bit 0)
    if (want == ROI_DOWN_SHARE && on(c->roi_share_rect) && (c->roi_down & 1u)) want = ROI_DOWN_SHARE_RECT;
    if (want == ROI_DOWN_SHARE_RECT && on(c->roi_share_fused_rect)) want = ROI_DOWN_SHARE_FUSED_RECT;
    // ... and where the plan shares anything, has the form and its longest table fits
    return roi_down_form(*plan, want);
}

// Down path (memory-bound kernels + small pointwise GEMMs): X (n, P, P) -> dout (n, P/16, P/16, f_deep)
// plan, form (tiled callers; ROI_DOWN_FULL: whole patches): the form roi_down_resolve gave for the pass; the patches are in the plan's
// class-major order, and what every launch computes and every stored tensor is copied into is the planner's answer for the form
// (roi_plan.h:RoiDownForm).  The two bits of TMAT_ROI_DOWN stay independent under every form: bit 0 gates the segment tables of the
// rectangle launches, bit 1 the tile tables of the fused separable layers.
// padval: from ROI_DOWN_CONST upwards the k all-constant patches of the pass are written behind X's n patches and run through the same
// launches as one more segment of whole patches
int unet_down_dev(Ctx *c, const float *X, int n, float *dout, hipStream_t s, const RoiPlan *plan, const float *padval, RoiDownForm form, bool quad,
                  bool quad_pool)
{
    if (n <= 0) return TMAT_OK;
    if (n > c->max_patches) { set_error("unet_down_dev: n > max_patches"); return TMAT_E_ARG; }
    if (!plan || n % plan->tiles_per_img != 0) form = ROI_DOWN_FULL;
    if (form >= ROI_DOWN_CONST && !padval) { set_error("unet_down_dev: the constant-ring form needs the pad values"); return TMAT_E_ARG; }
    const bool roi_b = form != ROI_DOWN_FULL && (c->roi_down & 1u);
    const int kimg = form != ROI_DOWN_FULL ? n / plan->tiles_per_img : 0;
    const int n_own = n;
    if (form >= ROI_DOWN_CONST) {
        launch_const_patches(padval, kimg, c->patch * c->patch, const_cast<float *>(X) + (size_t)n * c->patch * c->patch, s);
        n += kimg;              // every launch below runs the constant patches too
    }
    c->sep_tiles.clear();
    c->down_segs = c->down_seg_total = 0;
    RoiSegs sg{};
    // the segments of layer l of the down plan (null: full-frame)
    auto segs_of = [&](int l) -> const RoiSegs * {
        if (!roi_b) return nullptr;
        roi_down_segs(*plan, form, l, kimg, sg);
        c->down_segs = std::max(c->down_segs, sg.nseg);
        c->down_seg_total += sg.nseg;
        return &sg;
    };
    // of layer k of down block bi
    auto segs = [&](size_t bi, int k) -> const RoiSegs * { return segs_of(6 * (int)bi + k); };
    const int LD = 6 * (int)c->down.size();
    // TMAT_ROI_DOWN bit 1: the tile table of fused layer k (1 or 3) of down block bi.  dev null: the launch stays full-frame (no plan, bf16x3
    // weights, or every patch whole).  A table that could not be made clears tab_ok (the error is set)
    RoiEntry *ent = form != ROI_DOWN_FULL && (c->roi_down & 2u) ? roi_entry_of(c, plan) : nullptr;
    bool tab_ok = true;
    const RoiShareTab *shr = nullptr;
    if (form >= ROI_DOWN_SHARE && !(ent && (shr = roi_share_tab(ent, kimg, form)))) return TMAT_E_HIP;
    // what layer l's tensor t (C channels) is copied into after the launch that writes it, before its readers: the strips the constant
    // patches hold, then the items out of the neighbour patches
    auto copies = [&](float *t, int l, int C) -> bool {
        if (form < ROI_DOWN_CONST) return true;
        FillItems f;
        roi_down_const_items(*plan, form, l, kimg, f);
        if (!launch_const_fill(t, n_own, n, plan->down.res[l], C, f, s)) return false;
        if (!shr) return true;
        for (const RoiShareTab::Layer &sl : shr->layers)
            if (sl.layer == l && !launch_share_fill(t, n_own, plan->down.res[l], C, shr->nbr.data(), shr->nbr_dev, sl.items.data(), sl.dev, (int)sl.items.size(), s))
                return false;
        return true;
    };
    auto tiles = [&](size_t bi, int k, int H, bool f32) -> RoiTileTab {
        RoiTileTab t;
        t.full = t.n = n * (H / 16) * (H / 16);
        t.full_rep = t.n_rep = (long long)n_own * (H / 16) * (H / 16);
        if (ent && f32) {
            // the plain layer of a level in ROI_QUAD_LEVELS, the pooled layer (on the fused pooling kernel) of a level in
            // ROI_QUAD_POOL_LEVELS: its quadrant table where the pass runs that quadrant form
            const bool q = form >= ROI_DOWN_SHARE && (k == 1 ? quad && ((ROI_QUAD_LEVELS >> bi) & 1u)
                                                             : quad_pool && c->fused_pool && ((ROI_QUAD_POOL_LEVELS >> bi) & 1u));
            if (const RoiTileTab *made = roi_tile_tab(ent, 6 * (int)bi + k, kimg, form, q)) t = *made;
            else tab_ok = false;
        }
        // (the constant patches' whole tiles are not counted; a quadrant table reports its packed tiles)
        c->sep_tiles.push_back({t.dev ? t.n_rep : t.full_rep, t.full_rep});
        return t;
    };
    const int P = c->patch;
    float *b0 = c->buf[0], *b1 = c->buf[1], *b2 = c->buf[2], *b3 = c->buf[3];
    const int di = dout == c->dout[1] ? 1 : 0;
    c->dout_relu_ok[di] = false;
    // Block 0 on the wave-specialised separable kernel: the stem tensor is never materialised -- the first separable convolution's
    // producers recompute it from the patch (sepconv_ws_kernel<..., STEM>), and the stride-2 residual convolution, which samples the
    // even pixels only, reads those from stem_even_kernel's quarter-size tensor as a unit-stride 1x1 convolution.
    const bool stem_in_sep = c->stem_fused && !c->down.empty() && down_block_ws(c, 0) && c->down[0].cin == c->f0 &&
                             !(c->precision == TMAT_PRECISION_BF16X3 && c->sep_bf16);
    if (stem_in_sep) {
        launch_stem_even(X, n, P, P, c->stem_w, c->f0, c->stem_scale, c->stem_shift, b0, s, segs_of(form == ROI_DOWN_FULL ? 4 : roi_down_stem_layer(*plan, form)));     // the pixels block 0's residual 1x1 takes
        if (!copies(b0, LD, c->f0)) return TMAT_E_ARG;
    } else launch_stem(X, n, P, P, c->stem_w, c->f0, c->stem_scale, c->stem_shift, b0, s);
    int H = P / 2;
    for (size_t bi = 0; bi < c->down.size(); bi++) {
        auto &d = c->down[bi];
        // prev = b0 (n, H, H, cin)
        if (down_block_ws(c, bi)) {
            // fused separable kernels (sepconv_ws_kernels.hip): depthwise producers + MFMA consumers in one workgroup.
            // bf16x3 mode: the pointwise contraction on the split weights (bf16x6 keeps these layers in f32: three planes do not fit the LDS budget)
            const float *pw0 = d.pw[0], *pw1 = d.pw[1];
            int sprec = 0;
            if (c->precision == TMAT_PRECISION_BF16X3 && c->sep_bf16) {
                auto &mp = c->wsplit[c->precision];
                auto i0 = mp.find(d.pw[0]), i1 = mp.find(d.pw[1]);
                if (i0 != mp.end() && i1 != mp.end()) { pw0 = i0->second; pw1 = i1->second; sprec = 1; }
            }
            const bool stem_here = bi == 0 && stem_in_sep;
            const RoiTileTab t0 = tiles(bi, 1, H, sprec == 0), t1 = tiles(bi, 3, H, sprec == 0);
            if (!tab_ok) return TMAT_E_HIP;
            if (stem_here) {
                if (!launch_sepconv_ws_stem(X, n, H, H, d.cin, c->stem_w, c->stem_scale, c->stem_shift, d.dw[0], pw0, d.cout, d.scale[0], d.shift[0], 1, b2, s,
                                            t0.dev, t0.n, t0.quad)) return TMAT_E_ARG;
            } else if (!launch_sepconv_ws(b0, n, H, H, d.cin, bi > 0, d.dw[0], pw0, d.cout, d.scale[0], d.shift[0], 1, b2, s, sprec, t0.dev, t0.n, t0.quad)) return TMAT_E_ARG;
            if (!copies(b2, 6 * (int)bi + 1, d.cout)) return TMAT_E_ARG;
            ConvArgs r{};
            r.in = b0; r.N = n; r.h = H; r.w = H; r.Cin = d.cin; r.ksize = 1; r.stride = 2; r.W = d.res_w; r.Cout = d.cout;
            r.scale = nullptr; r.shift = d.res_b; r.out = b1;
            if (stem_here) { r.h = H / 2; r.w = H / 2; r.stride = 1; }      // b0 holds the even pixels only
            if (!conv(c, r, s, segs(bi, 4)) || !copies(b1, 6 * (int)bi + 4, d.cout)) return TMAT_E_ARG;
            float *nxt = bi + 1 == c->down.size() ? dout : b0;
            // (outside the residual's rectangle the pooled pixels take values nobody wrote and nobody reads; a tile the table skips leaves
            // its pixels and strips unwritten: a needed pooled pixel's 2 i .. 2 i + 2 lie in the layer's rectangle, strips included)
            if (c->fused_pool) {
                if (!launch_sepconv_pool_ws(b2, n, H, H, d.cout, 0, d.dw[1], pw1, d.cout, d.scale[1], d.shift[1], 0, b3, b1, nxt, s, sprec, segs(bi, 5),
                                            t1.dev, t1.n, t1.quad)) return TMAT_E_ARG;
            } else {
                if (!launch_sepconv_ws(b2, n, H, H, d.cout, 0, d.dw[1], pw1, d.cout, d.scale[1], d.shift[1], 0, b3, s, sprec, t1.dev, t1.n)) return TMAT_E_ARG;
                launch_maxpool_add(b3, n, H, H, d.cout, b1, nxt, s, nullptr, segs(bi, 5));
            }
            // (the fix-up pass may have written junk into pooled pixels of skipped tiles: the copies overwrite every one a consumer reads)
            if (!copies(nxt, 6 * (int)bi + 5, d.cout)) return TMAT_E_ARG;
            H /= 2;
            continue;
        }
        const int l0 = 6 * (int)bi;
        launch_dwconv(b0, n, H, H, d.cin, 1, d.dw[0], b1, s, segs(bi, 0));
        if (!copies(b1, l0, d.cin)) return TMAT_E_ARG;
        ConvArgs a{};
        a.in = b1; a.N = n; a.h = H; a.w = H; a.Cin = d.cin; a.relu_in = 0; a.ksize = 1; a.stride = 1;
        a.W = d.pw[0]; a.Cout = d.cout; a.scale = d.scale[0]; a.shift = d.shift[0]; a.resid = nullptr; a.rs = 0;
        a.relu_out = 1; a.out = b2;
        if (!conv(c, a, s, segs(bi, 1)) || !copies(b2, l0 + 1, d.cout)) return TMAT_E_ARG;
        launch_dwconv(b2, n, H, H, d.cout, 0, d.dw[1], b3, s, segs(bi, 2));
        if (!copies(b3, l0 + 2, d.cout)) return TMAT_E_ARG;
        a.in = b3; a.Cin = d.cout; a.W = d.pw[1]; a.scale = d.scale[1]; a.shift = d.shift[1]; a.relu_out = 0; a.out = b2;
        if (!conv(c, a, s, segs(bi, 3)) || !copies(b2, l0 + 3, d.cout)) return TMAT_E_ARG;
        ConvArgs r{};
        r.in = b0; r.N = n; r.h = H; r.w = H; r.Cin = d.cin; r.ksize = 1; r.stride = 2; r.W = d.res_w; r.Cout = d.cout;
        r.scale = nullptr; r.shift = d.res_b; r.out = b1;
        if (!conv(c, r, s, segs(bi, 4)) || !copies(b1, l0 + 4, d.cout)) return TMAT_E_ARG;
        const bool last = bi + 1 == c->down.size();
        float *dr = (last && c->relu_copy && dout == c->dout[di]) ? c->dout_relu[di] : nullptr;      // activated copy for the first up block
        launch_maxpool_add(b2, n, H, H, d.cout, b1, last ? dout : b0, s, dr, segs(bi, 5));
        // (the rectangle launches' form: the shared zone of the bottleneck tensor and of its activated copy comes from the neighbours)
        if (!copies(last ? dout : b0, l0 + 5, d.cout) || (dr && !copies(dr, l0 + 5, d.cout))) return TMAT_E_ARG;
        if (dr) c->dout_relu_ok[di] = true;
        H /= 2;
    }
    TMAT_HIP(hipGetLastError());
    return TMAT_OK;
}

// Up path (the MFMA-bound 3x3 transposed convolutions) + final conv: dout -> Y (n, P, P)

const RoiPlan *roi_find(const Ctx *c, const TileGeom &g)
{
    if (!g.order) return nullptr;
    for (const RoiEntry *e : c->roi_cache) if (e->order == g.order) return &e->plan;
    return nullptr;
}

const RoiPlan *roi_attach(Ctx *c, TileGeom &g)
{
    g.order = nullptr;
    if (!c->roi_on || g.tiles_per_img > c->max_patches || c->up.empty() || (int)c->up.size() > ROI_MAX_UP) return nullptr;
    for (RoiEntry *e : c->roi_cache)          // the tile tables of the other geometries go (entry points drain their streams before they return)
        if (!(e->plan.hh == g.hh && e->plan.ww == g.ww && e->plan.ws == g.ws)) e->free_tabs();
    for (const RoiEntry *e : c->roi_cache)
        if (e->plan.hh == g.hh && e->plan.ww == g.ww && e->plan.ws == g.ws) { g.order = e->order; return e->order ? &e->plan : nullptr; }
    RoiEntry *e = new RoiEntry();
    c->roi_cache.push_back(e);
    int chan[ROI_MAX_UP + 1];
    chan[0] = c->up[0].cin;
    for (size_t j = 0; j < c->up.size(); j++) chan[j + 1] = c->up[j].cout;
    if (!roi_make_plan(g.hh, g.ww, g.ws, (int)c->up.size(), chan, ROI_MAX_CLASSES, e->plan) || e->plan.n_classes == 0) {
        e->plan.hh = g.hh; e->plan.ww = g.ww; e->plan.ws = g.ws; e->plan.n_classes = 0;       // remembered: this geometry stays full-frame
        return nullptr;
    }
    e->plan.tight = c->roi_tight;
    e->plan.exact = c->roi_exact;
    if (c->roi_down && c->down.size() <= (size_t)ROI_MAX_DOWN) {      // the down-path tables (a geometry they do not take keeps the down path full-frame)
        int dchan[ROI_MAX_DOWN + 1];
        unsigned fused = 0;
        dchan[0] = c->f0;
        for (size_t b = 0; b < c->down.size(); b++) { dchan[b + 1] = c->down[b].cout; if (down_block_ws(c, b)) fused |= 1u << b; }
        roi_plan_down(e->plan, (int)c->down.size(), dchan, fused);
    }
    const RoiPlan &p = e->plan;
    std::vector<int4> tab(p.tiles_per_img);
    for (int t = 0; t < p.tiles_per_img; t++) tab[t] = make_int4(p.class_base[p.tile_class[t]], p.class_count[p.tile_class[t]], p.tile_rank[t], 0);
    // (a blocking copy into a fresh allocation, once per geometry and handle: nothing in flight reads it)
    if (!hip_ok(hipMalloc((void **)&e->order, tab.size() * sizeof(int4)), "hipMalloc(patch order)") ||
        !hip_ok(hipMemcpy(e->order, tab.data(), tab.size() * sizeof(int4), hipMemcpyHostToDevice), "hipMemcpy(patch order)")) {
        if (e->order) hipFree(e->order);
        e->order = nullptr; e->plan.n_classes = 0;
        return nullptr;
    }
    g.order = e->order;
    return &e->plan;
}

int unet_up_dev(Ctx *c, const float *dout, int n, float *Y, hipStream_t s, const RoiPlan *plan)
{
    if (n <= 0) return TMAT_OK;
    if (plan && (plan->n_classes <= 0 || plan->n_up != (int)c->up.size() || n % plan->tiles_per_img)) { set_error("unet_up_dev: region plan does not fit the batch"); return TMAT_E_ARG; }
    const int kimg = plan ? n / plan->tiles_per_img : 0;
    RoiSegs sg{};
    auto segs = [&](int l) -> const RoiSegs * { if (!plan) return nullptr; sg = roi_segs(*plan, l, kimg); return &sg; };
    // S = stored tensor at resolution Hs; logical block input = Up^up(S).  `dout` is never recycled.
    const float *S = dout;
    int Hs = c->patch >> (1 + c->down.size()), up = 0;
    float *t1 = c->ubuf[0], *rr = c->ubuf[1];
    int so_idx = 2;
    // S_act: the activated copy of S when its producer wrote one (the block's first convolution then needs no ReLU on load)
    const int di = dout == c->dout[1] ? 1 : 0;
    const float *S_act = (c->relu_copy && dout == c->dout[di] && c->dout_relu_ok[di]) ? c->dout_relu[di] : nullptr;
    for (size_t j = 0; j < c->up.size(); j++) {
        auto &u = c->up[j];
        float *so = c->ubuf[so_idx];
        ConvArgs a{};
        a.in = S_act ? S_act : S; a.N = n; a.h = Hs; a.w = Hs; a.Cin = u.cin; a.relu_in = S_act ? 0 : 1; a.ksize = 3; a.stride = 1;
        a.W = u.ct[0];
        if (up) { a.ksize = 2; a.W = u.ct_sub; }      // 4 taps per output parity class instead of 9
        a.Cout = u.cout; a.scale = u.scale[0]; a.shift = u.shift[0]; a.relu_out = 1; a.out = t1;
        if (!conv(c, a, s, segs(3 * (int)j))) return TMAT_E_ARG;
        ConvArgs r{};
        r.in = S; r.N = n; r.h = Hs; r.w = Hs; r.Cin = u.cin; r.ksize = 1; r.stride = 1; r.W = u.res_w; r.Cout = u.cout;
        r.scale = nullptr; r.shift = u.res_b; r.out = rr;
        if (!conv(c, r, s, segs(3 * (int)j + 1))) return TMAT_E_ARG;
        const int Hl = Hs << up;
        ConvArgs b{};
        b.in = t1; b.N = n; b.h = Hl; b.w = Hl; b.Cin = u.cout; b.relu_in = 0; b.ksize = 3; b.stride = 1;
        b.W = u.ct[1]; b.Cout = u.cout; b.scale = u.scale[1]; b.shift = u.shift[1]; b.resid = rr; b.rs = up; b.relu_out = 0;
        b.out = so;
        // the next block's first convolution reads relu(so): written here as a second output (the last block's output feeds the final conv as is)
        float *so_act = (c->relu_copy && j + 1 < c->up.size()) ? c->urelu[j & 1] : nullptr;
        b.out_relu = so_act;
        if (!conv(c, b, s, segs(3 * (int)j + 2))) return TMAT_E_ARG;
        S = so; S_act = so_act; so_idx = so_idx == 2 ? 3 : 2;
        Hs = Hl; up = 1;
    }
    launch_final(S, n, Hs, Hs, c->f_last, c->final_w, c->final_b, Y, s, segs(3 * (int)c->up.size()));
    TMAT_HIP(hipGetLastError());
    return TMAT_OK;
}

// n may exceed max_patches (an image that needs more patches than the activation workspace holds): the patch list
// is then walked in chunks of max_patches, all on stream `s`
int unet_forward_dev(Ctx *c, const float *X, int n, float *Y, hipStream_t s)
{
    const size_t pp = (size_t)c->patch * c->patch;
    for (int i0 = 0; i0 < n; i0 += c->max_patches) {
        const int k = std::min(c->max_patches, n - i0);
        int rc = unet_down_dev(c, X + (size_t)i0 * pp, k, c->dout[0], s);
        if (rc) return rc;
        rc = unet_up_dev(c, c->dout[0], k, Y + (size_t)i0 * pp, s);
        if (rc) return rc;
    }
    return TMAT_OK;
}

// patch_in / patch_out hold max_patches patches; an image that needs more gets larger ones (2 x 0.41 MB per patch).
// Only called between entry points (nothing in flight uses the old buffers).
int ensure_patch_io(Ctx *c, int n_patches)
{
    if (n_patches <= c->patch_cap) return TMAT_OK;
    TMAT_HIP(hipStreamSynchronize(c->stream));
    TMAT_HIP(hipStreamSynchronize(c->stream2));
    for (float *p : {c->patch_in, c->patch_in2, c->patch_out}) c->ws.release(p);
    c->patch_in = c->patch_in2 = c->patch_out = nullptr;
    c->patch_cap = 0;
    const size_t bytes = (size_t)c->patch * c->patch * n_patches * sizeof(float);
    c->patch_in = (float *)c->ws.dev(bytes + (size_t)c->patch * c->patch * c->const_cap * sizeof(float), "hipMalloc(patch_in)");
    c->patch_out = (float *)c->ws.dev(bytes, "hipMalloc(patch_out)");
    if (!c->patch_in || !c->patch_out) return TMAT_E_HIP;
    c->patch_cap = n_patches;
    return TMAT_OK;
}

// predict_img_with_smooth_windowing on device: x_dev (n, hh, ww) f32 -> pred_dev (n, hh, ww) f64
int predict_smooth_dev(Ctx *c, float *x_dev, int n, int hh, int ww, double *pred_dev)
{
    if (c->norm_on) launch_norm_f32(x_dev, (size_t)n * hh * ww, c->norm_mean, c->norm_std, c->stream);
    const int P = c->patch;
    TileGeom g = make_geom(hh, ww, P);
    const RoiPlan *plan = roi_attach(c, g);       // region form of the up path (null: oversize image, or TMAT_ROI=0)
    const int per_pass = std::max(1, c->max_patches / g.tiles_per_img);
    { int rc = ensure_patch_io(c, per_pass * g.tiles_per_img); if (rc) return rc; }
    size_t need_pv = (size_t)std::min(n, per_pass) * 2 * sizeof(float);
    if (need_pv > c->scratch_bytes) { set_error("predict_smooth: scratch too small"); return TMAT_E_ARG; }
    float *mn = (float *)c->scratch, *mx = mn + std::min(n, per_pass);
    for (int i0 = 0; i0 < n; i0 += per_pass) {
        int k = std::min(per_pass, n - i0);
        const float *xi = x_dev + (size_t)i0 * hh * ww;
        launch_minmax_f32(xi, k, (size_t)hh * ww, mn, mx, c->stream);
        launch_extract_tiles(xi, mn, k, g, c->patch_in, c->stream);
        // (the constant-ring form only on request: the default launches of this entry point are pinned to the dependency plan's tiles)
        int rc = plan ? unet_down_dev(c, c->patch_in, k * g.tiles_per_img, c->dout[0], c->stream, plan, mn, roi_down_resolve(c, plan, k, true, false), roi_quad_on(c, false), roi_quad_pool_on(c, false))
                      : unet_forward_dev(c, c->patch_in, k * g.tiles_per_img, c->patch_out, c->stream);
        if (!rc && plan) rc = unet_up_dev(c, c->dout[0], k * g.tiles_per_img, c->patch_out, c->stream, plan);
        if (rc) return rc;
        launch_blend(c->patch_out, c->win1d, k, g, pred_dev + (size_t)i0 * hh * ww, c->stream);
    }
    TMAT_HIP(hipGetLastError());
    return TMAT_OK;
}

// smooth_tiled_predictions.py:26-41 in f64.  scipy.signal.windows.triang(M): (2 n - 1) / M for even M, 2 n / (M + 1) for odd M,
// n = 1 .. (M + 1) / 2, mirrored (the odd form without repeating its centre); np.average is np.mean: numpy's pairwise sum over ws.
std::vector<double> spline_window_host(int ws)
{
    std::vector<double> tri(ws), wind(ws);
    for (int i = 0; i < (ws + 1) / 2; i++) {
        tri[i] = ws % 2 == 0 ? (2.0 * (i + 1) - 1.0) / ws : (2.0 * (i + 1)) / (ws + 1.0);
        tri[ws - 1 - i] = tri[i];
    }
    const int isec = ws / 4;
    for (int i = 0; i < ws; i++) {
        double a2 = std::fabs(2 * tri[i]); double outer = (a2 * a2) / 2;
        if (i >= isec && i < ws - isec) outer = 0;
        double b2 = std::fabs(2 * (tri[i] - 1)); double inner = 1 - (b2 * b2) / 2;
        if (i < isec || i >= ws - isec) inner = 0;
        wind[i] = inner + outer;
    }
    const double avg = numpy_pairwise_sum(wind.data(), ws) / ws;
    for (int i = 0; i < ws; i++) wind[i] = wind[i] / avg;
    return wind;
}

}  // namespace tmat

using namespace tmat;

extern "C" {

const char *tmat_last_error(void)
{
    static thread_local std::string copy;       // stays valid for the caller until its next call on this thread
    std::lock_guard<std::mutex> lk(g_err_mu);
    copy = g_err;
    return copy.c_str();
}
int tmat_version(void) { return 0x000100; }

// A handle without a model: device + stream only, for the entry points that need no weights (tmat_zproj_*,
// tmat_filter_edt_batch, tmat_finish_batch).  Model entry points refuse it.
int tmat_create_plain(int device_id, tmat_handle *out)
{
    if (!out) { set_error("tmat_create_plain: null argument"); return TMAT_E_ARG; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("tmat_create_plain: no HIP device available (libtmat_hip has no CPU fallback)");
        return TMAT_E_HIP;
    }
    if (device_id < 0 || device_id >= ndev) { set_error("tmat_create_plain: bad device id"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(device_id));
    Ctx *c = new Ctx();
    c->device = device_id;
    if (!hip_ok(hipStreamCreate(&c->stream), "hipStreamCreate")) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    { const int rc = resnet_precision_from_env(c); if (rc) { tmat_destroy((tmat_handle)c); return rc; } }
    *out = (tmat_handle)c;
    return TMAT_OK;
}

int tmat_create(int device_id, const void *weights_blob, size_t n_bytes, int max_patches, tmat_handle *out)
{
    if (!out || !weights_blob) { set_error("tmat_create: null argument"); return TMAT_E_ARG; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("tmat_create: no HIP device available (libtmat_hip has no CPU fallback)");
        return TMAT_E_HIP;
    }
    if (device_id < 0 || device_id >= ndev) { set_error("tmat_create: bad device id"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(device_id));
    std::map<std::string, Tensor> m;
    int patch = 0;
    if (!parse_blob(weights_blob, n_bytes, m, patch)) return TMAT_E_WEIGHTS;
    // a blob whose convolutions no kernel takes is refused here, with the rule, before anything is allocated
    const UnetSwitches sw = unet_switches_from_env();
    bool narrow = false;
    {
        ModelShape ms;
        std::vector<ModelLayer> layers;
        if (!model_shape(m, patch, ms) || !model_layers(ms, sw, layers)) return TMAT_E_WEIGHTS;
        for (const ModelLayer &l : layers) narrow = narrow || l.launcher == 1;
    }
    Ctx *c = new Ctx();
    c->device = device_id;
    c->patch = patch;
    c->max_patches = max_patches > 0 ? max_patches : 400;
    c->narrow = narrow;
    c->fused_sep = sw.fused_sep; c->fused_pool = sw.fused_pool; c->stem_fused = sw.stem_fused;
    if (const char *e = getenv("TMAT_ROI")) c->roi_on = atoi(e) != 0;
    if (const char *e = getenv("TMAT_ROI_TIGHT")) c->roi_tight = atoi(e) != 0;
    if (const char *e = getenv("TMAT_ROI_EXACT")) c->roi_exact = atoi(e) != 0;
    if (const char *e = getenv("TMAT_ROI_DOWN")) {
        // a bit mask of bit 0 (the unfused level and the small kernels) and bit 1 (the fused separable layers' tile tables): anything else
        // is an error, not a silent full-frame run
        if (strcmp(e, "0") && strcmp(e, "1") && strcmp(e, "2") && strcmp(e, "3")) { set_error("tmat_create: TMAT_ROI_DOWN must be 0, 1, 2 or 3"); delete c; return TMAT_E_ARG; }
        c->roi_down = (unsigned)atoi(e);
    }
    if (const char *e = getenv("TMAT_ROI_CONST")) {
        if (strcmp(e, "0") && strcmp(e, "1")) { set_error("tmat_create: TMAT_ROI_CONST must be 0 or 1"); delete c; return TMAT_E_ARG; }
        c->roi_const = atoi(e);
    }
    if (const char *e = getenv("TMAT_ROI_SHARE")) {
        if (strcmp(e, "0") && strcmp(e, "1")) { set_error("tmat_create: TMAT_ROI_SHARE must be 0 or 1"); delete c; return TMAT_E_ARG; }
        c->roi_share = atoi(e);
    }
    if (const char *e = getenv("TMAT_ROI_SHARE_RECT")) {
        if (strcmp(e, "0") && strcmp(e, "1")) { set_error("tmat_create: TMAT_ROI_SHARE_RECT must be 0 or 1"); delete c; return TMAT_E_ARG; }
        c->roi_share_rect = atoi(e);
    }
    if (const char *e = getenv("TMAT_ROI_SHARE_FUSED_RECT")) {
        if (strcmp(e, "0") && strcmp(e, "1")) { set_error("tmat_create: TMAT_ROI_SHARE_FUSED_RECT must be 0 or 1"); delete c; return TMAT_E_ARG; }
        c->roi_share_fused_rect = atoi(e);
    }
    if (const char *e = getenv("TMAT_ROI_QUAD")) {
        if (strcmp(e, "0") && strcmp(e, "1")) { set_error("tmat_create: TMAT_ROI_QUAD must be 0 or 1"); delete c; return TMAT_E_ARG; }
        c->roi_quad = atoi(e);
    }
    if (const char *e = getenv("TMAT_ROI_QUAD_POOL")) {
        if (strcmp(e, "0") && strcmp(e, "1")) { set_error("tmat_create: TMAT_ROI_QUAD_POOL must be 0 or 1"); delete c; return TMAT_E_ARG; }
        c->roi_quad_pool = atoi(e);
    }
    // room for the all-constant patches of a pass behind its patches (tmat_ctx.h): the down-path workspaces and the input buffers only
    c->const_cap = c->roi_const == 0 ? 0 : std::max(4, c->max_patches / 64);
    if (const char *e = getenv("TMAT_SEP_BF16")) c->sep_bf16 = atoi(e) != 0;
    const char *prec_env = getenv("TMAT_PRECISION");
    if (prec_env && strcmp(prec_env, "f32") && strcmp(prec_env, "bf16x3") && strcmp(prec_env, "bf16x6")) {
        set_error("tmat_create: TMAT_PRECISION must be f32, bf16x3 or bf16x6");
        delete c;
        return TMAT_E_ARG;
    }
    { const int rc = resnet_precision_from_env(c); if (rc) { delete c; return rc; } }
    if (const char *e = getenv("TMAT_DMT_DEVICE")) c->dmt_device = atoi(e) != 0;
    if (const char *e = getenv("TMAT_DMT_SWEEP_DEVICE")) c->dmt_sweep_device = atoi(e) != 0;
    if (const char *e = getenv("TMAT_PRE_STREAM")) c->pre_side = atoi(e) != 0;
    if (const char *e = getenv("TMAT_THIN_DEVICE")) c->thin_device = atoi(e) != 0;
    // the UNet stream gets the highest priority, the side stream of the post-processing stages (thinning rounds, finish,
    // DMT front end: many short launches that only have to be done before the next pass ends) the lowest: they fill the
    // gaps instead of taking workgroup slots from the MFMA kernels
    int prio_least = 0, prio_greatest = 0;
    hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (!hip_ok(hipStreamCreateWithPriority(&c->stream, hipStreamDefault, prio_greatest), "hipStreamCreate") || !build_model(c, m)) { tmat_destroy((tmat_handle)c); return TMAT_E_WEIGHTS; }
    // activation workspace: per patch (P/2)^2 * f0 floats for buf0/buf1 and twice that for buf2/buf3
    const size_t unit = (size_t)(patch / 2) * (patch / 2) * c->f0;
    const size_t sizes[4] = {unit, unit, 2 * unit, 2 * unit};
    const size_t down_cap = (size_t)c->max_patches + c->const_cap;
    auto dev_f32 = [c](size_t bytes, const char *what) { return (float *)c->ws.dev(bytes, what); };
    for (int i = 0; i < 4; i++)
        if (!(c->buf[i] = dev_f32(sizes[i] * down_cap * sizeof(float), "hipMalloc(activations)"))) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    // up-path buffers: t1 (unit), hoisted residual (unit/4), block outputs alternate (unit/2, unit); down-path output x2
    const size_t usizes[4] = {unit, unit / 4, unit / 2, unit};
    for (int i = 0; i < 4; i++)
        if (!(c->ubuf[i] = dev_f32(usizes[i] * c->max_patches * sizeof(float), "hipMalloc(up buffers)"))) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    const size_t dsz = (size_t)(patch >> (1 + c->down.size())) * (patch >> (1 + c->down.size())) * c->up[0].cin;
    const size_t dout_bytes = dsz * down_cap * sizeof(float);
    for (int i = 0; i < 2; i++)
        if (!(c->dout[i] = dev_f32(dout_bytes, "hipMalloc(dout)"))) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    if (const char *e = getenv("TMAT_RELU_COPY")) c->relu_copy = atoi(e) != 0;
    if (c->relu_copy) {
        // up block j's output has (P/16 << j)^2 x cout_j values per patch: the larger of the even / odd blocks sizes each buffer
        size_t need[2] = {0, 0};
        for (size_t j = 0; j + 1 < c->up.size(); j++) {
            const size_t side = (size_t)(patch >> (1 + c->down.size())) << j;
            need[j & 1] = std::max(need[j & 1], side * side * c->up[j].cout);
        }
        for (int i = 0; i < 2; i++)
            if (!(c->dout_relu[i] = dev_f32(dout_bytes, "hipMalloc(dout_relu)")) ||
                (need[i] && !(c->urelu[i] = dev_f32(need[i] * c->max_patches * sizeof(float), "hipMalloc(urelu)")))) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    }
    if (!hip_ok(hipStreamCreate(&c->stream2), "hipStreamCreate(2)") || !hip_ok(hipStreamCreateWithPriority(&c->stream3, hipStreamDefault, prio_least), "hipStreamCreate(3)")) {
        tmat_destroy((tmat_handle)c); return TMAT_E_HIP;
    }
    for (int i = 0; i < 2; i++)
        if (!hip_ok(hipEventCreateWithFlags(&c->ev_down[i], hipEventDisableTiming), "hipEventCreate") ||
            !hip_ok(hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming), "hipEventCreate") ||
            !hip_ok(hipEventCreateWithFlags(&c->ev_pre[i], hipEventDisableTiming), "hipEventCreate") ||
            !hip_ok(hipEventCreateWithFlags(&c->ev_blend[i], hipEventDisableTiming), "hipEventCreate")) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    const size_t pp = (size_t)patch * patch * c->max_patches * sizeof(float);
    c->scratch_bytes = 64 << 20;
    for (int i = 0; i < 2 && c->const_cap; i++)
        if (!(c->padval[i] = dev_f32((size_t)c->const_cap * sizeof(float), "hipMalloc(pad values)"))) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    if (!(c->patch_in = dev_f32(pp + (size_t)patch * patch * c->const_cap * sizeof(float), "hipMalloc(patch_in)")) || !(c->patch_out = dev_f32(pp, "hipMalloc(patch_out)")) ||
        !(c->scratch = c->ws.dev(c->scratch_bytes, "hipMalloc(scratch)"))) { tmat_destroy((tmat_handle)c); return TMAT_E_HIP; }
    c->patch_cap = c->max_patches;
    // squared-spline window (smooth_tiled_predictions.py:26-41), f64, on host then uploaded
    {
        const int ws = patch;
        const std::vector<double> wind = spline_window_host(ws);
        if (!hip_ok(hipMalloc((void **)&c->win1d, ws * sizeof(double)), "hipMalloc(win)") ||
            !hip_ok(hipMemcpy(c->win1d, wind.data(), ws * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(win)")) {
            tmat_destroy((tmat_handle)c); return TMAT_E_HIP;
        }
        c->win_host = wind;
    }
    *out = (tmat_handle)c;
    if (prec_env && strcmp(prec_env, "f32")) {
        const int rc = tmat_set_precision((tmat_handle)c, !strcmp(prec_env, "bf16x3") ? TMAT_PRECISION_BF16X3 : TMAT_PRECISION_BF16X6);
        if (rc) { tmat_destroy((tmat_handle)c); *out = nullptr; return rc; }
    }
    return TMAT_OK;
}

void tmat_destroy(tmat_handle h)
{
    Ctx *c = (Ctx *)h;
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (void *p : c->owned) hipFree(p);
    if (c->stream2) hipStreamSynchronize(c->stream2);
    for (int i = 0; i < 2; i++) { if (c->ev_down[i]) hipEventDestroy(c->ev_down[i]); if (c->ev_up[i]) hipEventDestroy(c->ev_up[i]); if (c->ev_pre[i]) hipEventDestroy(c->ev_pre[i]); if (c->ev_blend[i]) hipEventDestroy(c->ev_blend[i]); }
    if (c->stream2) hipStreamDestroy(c->stream2);
    if (c->stream3) { hipStreamSynchronize(c->stream3); hipStreamDestroy(c->stream3); }
    c->ws.free_all();
    c->smooth.close();
    for (hipEvent_t e : c->smooth.ev) if (e) hipEventDestroy(e);
    for (RoiEntry *e : c->roi_cache) { e->free_tabs(); if (e->order) hipFree(e->order); delete e; }
    if (c->win1d) hipFree(c->win1d);
    if (c->ma_table) hipFree(c->ma_table);
    if (c->se_table) hipFree(c->se_table);
    for (void *p : c->tool_ws) if (p) hipFree(p);
    for (auto &b : c->ws_pool) hipFree(b.second);
    c->stack_host.free_all();
    for (auto &g : c->gauss_dev) hipFree(g.second);
    for (auto &m : c->resnets) for (void *p : m.owned) hipFree(p);
    c->free_pass();
    for (auto &e : c->ev_open) { hipEventDestroy(e.e0); hipEventDestroy(e.e1); }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int tmat_sync(tmat_handle h)
{
    Ctx *c = (Ctx *)h;
    if (!c) { set_error("null handle"); return TMAT_E_ARG; }
    if (c->stream2) TMAT_HIP(hipStreamSynchronize(c->stream2));
    if (c->stream3) TMAT_HIP(hipStreamSynchronize(c->stream3));
    TMAT_HIP(hipStreamSynchronize(c->stream));
    return TMAT_OK;
}

int tmat_unet_predict(tmat_handle h, const float *x, int n, float *y)
{
    Ctx *c = (Ctx *)h;
    if (c && !has_model(c)) { set_error("tmat_unet_predict: this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (!c || !x || !y || n < 0) { set_error("tmat_unet_predict: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t per = (size_t)c->patch * c->patch;
    DevScope mem(c->ws_pool, c->stream);       // the handle's patch buffers; the scope only carries the copies
    for (int i0 = 0; i0 < n; i0 += c->max_patches) {
        int k = std::min(c->max_patches, n - i0);
        if (!mem.h2d(c->patch_in, x + i0 * per, k * per * sizeof(float))) return TMAT_E_HIP;
        int rc = unet_forward_dev(c, c->patch_in, k, c->patch_out, c->stream);
        if (rc) return rc;
        mem.d2h(y + i0 * per, c->patch_out, k * per * sizeof(float));
        if (mem.finish()) return TMAT_E_HIP;
    }
    return TMAT_OK;
}

int tmat_predict_smooth(tmat_handle h, const float *x, int n, int hh, int ww, double *pred)
{
    Ctx *c = (Ctx *)h;
    if (c && !has_model(c)) { set_error("tmat_predict_smooth: this handle has no model (tmat_create_plain)"); return TMAT_E_ARG; }
    if (!c || !x || !pred || n < 0 || hh <= 0 || ww <= 0) { set_error("tmat_predict_smooth: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t per = (size_t)hh * ww;
    DevScope mem(c->ws_pool, c->stream);
    float *xd = mem.alloc_from(x, n * per);
    double *pd = mem.alloc<double>(n * per, "hipMalloc(pred)");
    if (!mem.ok) return TMAT_E_HIP;
    int rc = predict_smooth_dev(c, xd, n, hh, ww, pd);
    if (rc) return rc;
    mem.d2h(pred, pd, n * per * sizeof(double));
    return mem.finish();
}

int tmat_dev_alloc(tmat_handle h, size_t bytes, void **dev_ptr)
{
    Ctx *c = (Ctx *)h;
    if (!c || !dev_ptr) { set_error("tmat_dev_alloc: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    TMAT_HIP(hipMalloc(dev_ptr, bytes));
    return TMAT_OK;
}
int tmat_dev_free(tmat_handle h, void *dev_ptr)
{
    Ctx *c = (Ctx *)h;
    if (!c) { set_error("null handle"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    TMAT_HIP(hipFree(dev_ptr));
    return TMAT_OK;
}
int tmat_dev_upload(tmat_handle h, void *dev_dst, const void *host_src, size_t bytes)
{
    Ctx *c = (Ctx *)h;
    if (!c || !dev_dst || !host_src) { set_error("tmat_dev_upload: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    DevScope mem(c->ws_pool, c->stream);
    mem.h2d(dev_dst, host_src, bytes);
    return mem.finish();
}
int tmat_dev_download(tmat_handle h, void *host_dst, const void *dev_src, size_t bytes)
{
    Ctx *c = (Ctx *)h;
    if (!c || !host_dst || !dev_src) { set_error("tmat_dev_download: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    DevScope mem(c->ws_pool, c->stream);
    mem.d2h(host_dst, dev_src, bytes);
    return mem.finish();
}

int tmat_set_input_depth(tmat_handle h, int bits)
{
    Ctx *c = (Ctx *)h;
    if (!c || (bits != 8 && bits != 16)) { set_error("tmat_set_input_depth: bits must be 8 or 16"); return TMAT_E_ARG; }
    c->input_sat = bits == 8 ? 255.f : 65535.f;
    return TMAT_OK;
}

int tmat_set_input_norm(tmat_handle h, int on, double mean, double sd)
{
    Ctx *c = (Ctx *)h;
    if (!c || (on && !(sd != 0.0))) { set_error("tmat_set_input_norm: bad argument (norm_std must not be 0)"); return TMAT_E_ARG; }
    c->norm_on = on != 0;
    c->norm_mean = (float)mean;
    c->norm_std = (float)sd;
    return TMAT_OK;
}

int tmat_set_precision(tmat_handle h, int mode)
{
    Ctx *c = (Ctx *)h;
    if (!c || !has_model(c) || (mode != TMAT_PRECISION_F32 && mode != TMAT_PRECISION_BF16X3 && mode != TMAT_PRECISION_BF16X6)) {
        set_error("tmat_set_precision: needs a model handle and mode TMAT_PRECISION_F32, TMAT_PRECISION_BF16X3 or TMAT_PRECISION_BF16X6");
        return TMAT_E_ARG;
    }
    if (mode != TMAT_PRECISION_F32 && c->narrow) {
        set_error("tmat_set_precision: this model has layers of 16 or 32 channels, which run on the narrow convolution kernel in f32 only");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    if (mode != TMAT_PRECISION_F32) {
        auto &mp = c->wsplit[mode];
        // bf16x6 keeps the fused separable layers in f32 (three planes do not fit their LDS budget): no split copy of their pointwise weights
        std::vector<const float *> skip;
        if (mode == TMAT_PRECISION_BF16X6)
            for (size_t bi = 0; bi < c->down.size(); bi++)
                if (down_block_ws(c, bi)) { skip.push_back(c->down[bi].pw[0]); skip.push_back(c->down[bi].pw[1]); }
        for (auto &kv : c->conv_w_host) {
            if (mp.count(kv.first) || std::find(skip.begin(), skip.end(), kv.first) != skip.end()) continue;
            float *dev = nullptr;
            if (!upload(c, split_bf16(kv.second.w, mode + 1), &dev)) return TMAT_E_HIP;
            mp[kv.first] = dev;
        }
    }
    { const int rc = tmat_sync(h); if (rc) return rc; }      // all three streams: nothing in flight reads the old mode's weights
    c->precision = mode;
    return TMAT_OK;
}

// every workspace the handle retains between calls: the handle-lifetime list, the per-pass buffers, the side tools' slots and the pool
static std::vector<WsEnt> held_blocks(const Ctx *c)
{
    std::vector<WsEnt> all(c->ws.begin(), c->ws.end());
    all.insert(all.end(), c->pass.ws.begin(), c->pass.ws.end());
    for (int i = 0; i < N_TOOL_WS; i++) if (c->tool_ws[i]) all.push_back({c->tool_ws[i], c->tool_ws_bytes[i], false});
    for (auto &b : c->ws_pool) all.push_back({b.second, b.first, false});
    all.insert(all.end(), c->stack_host.begin(), c->stack_host.end());
    return all;
}

// Test-only (tests/test_gpu_poison.py): fill every scratch workspace of the handle -- the activation ping-pong sets, the pooled-tile
// strips that live in them, patch_in / patch_out, the scratch block and every per-pass device / pinned buffer -- with `byte_pattern`
// (0xFF: NaN as f32 / f64, -1 as int).  Weights, the spline window and the Lanczos tables are constants and stay.  A forward or a pass
// that reads a location it has not written in the same call then produces NaNs or a mismatch against the oracle deterministically,
// instead of depending on what a recycled allocation happens to hold.
int tmat_debug_poison(tmat_handle h, int byte_pattern)
{
    Ctx *c = (Ctx *)h;
    if (!c) { set_error("null handle"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    { const int rc = tmat_sync(h); if (rc) return rc; }
    std::vector<WsEnt> all = held_blocks(c);
    for (const WsEnt &e : all) {
        if (e.host) memset(e.p, byte_pattern, e.bytes);
        else TMAT_HIP(hipMemsetAsync(e.p, byte_pattern, e.bytes, c->stream));
    }
    TMAT_HIP(hipStreamSynchronize(c->stream));
    return TMAT_OK;
}

// Test-only (tests/test_gpu_held_memory.py): bytes of the workspaces tmat_debug_poison fills, device and pinned
int tmat_debug_held_bytes(tmat_handle h, size_t *device_bytes, size_t *pinned_bytes)
{
    Ctx *c = (Ctx *)h;
    if (!c || !device_bytes || !pinned_bytes) { set_error("tmat_debug_held_bytes: bad argument"); return TMAT_E_ARG; }
    *device_bytes = *pinned_bytes = 0;
    for (const WsEnt &e : held_blocks(c)) *(e.host ? pinned_bytes : device_bytes) += e.bytes;
    return TMAT_OK;
}

// Test-only (tests/test_gpu_roi_sep.py): planned and full tile counts of the fused separable launches of the last down pass; a launch
// in quadrant form reports its packed tiles as planned
int tmat_debug_sep_tiles(tmat_handle h, int cap, int *n, long long *planned, long long *full)
{
    Ctx *c = (Ctx *)h;
    if (!c || !n || cap < 0 || (cap > 0 && (!planned || !full))) { set_error("tmat_debug_sep_tiles: bad argument"); return TMAT_E_ARG; }
    *n = (int)c->sep_tiles.size();
    for (int i = 0; i < *n && i < cap; i++) { planned[i] = c->sep_tiles[i].first; full[i] = c->sep_tiles[i].second; }
    return TMAT_OK;
}

// Test-only (tests/test_gpu_sep_quads.py): ONE plain fused separable launch in quadrant form on host buffers with the caller's quadrant
// list (full-frame ids n QPP + qy QW + qx, any order, any patches; padded here to a multiple of 4 by repeating the last id).  x: (n, hh, ww,
// cin), or with the stem's weights (all three or none; relu_in 0) the single-channel patches (n, 2 hh, 2 ww).  dw9 [9][cin], pw in the Keras
// layout (cin, cout).  The caller fills out (n, hh, ww, cout): words of quadrants not listed come back as they went in.
int tmat_debug_sepconv_quads(tmat_handle hd, const float *x, int n, int hh, int ww, int cin, int relu_in, const float *dw9, const float *pw, int cout,
                             const float *scale, const float *shift, int relu_out, const float *stem_w, const float *stem_scale,
                             const float *stem_shift, const int *quads, int n_quads, float *out)
{
    Ctx *c = (Ctx *)hd;
    const bool stem = stem_w != nullptr;
    if (!c || !x || !dw9 || !pw || !scale || !shift || !quads || !out || n < 1 || n_quads < 1 || n_quads > (1 << 24) || hh < 16 || ww < 16 || cin < 1 ||
        cout < 1 || stem != (stem_scale != nullptr) || stem != (stem_shift != nullptr) || (stem && relu_in) || !sepconv_ws_supported(hh, ww, cin, cout) ||
        (long long)n * hh * ww * std::max(cin, cout) > 0x3fffffffLL) {
        set_error("tmat_debug_sepconv_quads: bad argument");
        return TMAT_E_ARG;
    }
    const long long nq = (long long)n * (hh / 8) * (ww / 8);
    std::vector<int> ids(quads, quads + n_quads);
    for (int id : ids) if (id < 0 || id >= nq) { set_error("tmat_debug_sepconv_quads: a quadrant id lies outside the tensor"); return TMAT_E_ARG; }
    while (ids.size() % 4) ids.push_back(ids.back());
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    const size_t nx = stem ? (size_t)n * hh * ww * 4 : (size_t)n * hh * ww * cin, no = (size_t)n * hh * ww * cout;
    std::vector<float> wk = k_contiguous(pw, 1, cin, cout);
    const size_t nw = wk.size();
    const float *hw = mem.keep(std::move(wk));
    const size_t n_ids = ids.size();
    const int *hid = mem.keep(std::move(ids));
    float *dx = mem.alloc_from(x, nx), *dd = mem.alloc_from(dw9, (size_t)9 * cin), *dw = mem.alloc_from(hw, nw);
    float *dsc = mem.alloc_from(scale, cout), *dsh = mem.alloc_from(shift, cout), *dout = mem.alloc_from((const float *)out, no);
    float *sw = stem ? mem.alloc_from(stem_w, (size_t)9 * cin) : nullptr, *ssc = stem ? mem.alloc_from(stem_scale, cin) : nullptr;
    float *ssh = stem ? mem.alloc_from(stem_shift, cin) : nullptr;
    int *dq = mem.alloc_from(hid, n_ids);
    if (!mem.ok) return TMAT_E_HIP;
    const bool ok = stem ? launch_sepconv_ws_stem(dx, n, hh, ww, cin, sw, ssc, ssh, dd, dw, cout, dsc, dsh, relu_out != 0, dout, s, dq, (int)(n_ids / 4), true)
                         : launch_sepconv_ws(dx, n, hh, ww, cin, relu_in != 0, dd, dw, cout, dsc, dsh, relu_out != 0, dout, s, 0, dq, (int)(n_ids / 4), true);
    if (!ok) return TMAT_E_ARG;
    mem.check(hipGetLastError(), "tmat_debug_sepconv_quads launch");
    mem.d2h(out, dout, no * sizeof(float));
    if (mem.finish()) return TMAT_E_HIP;
    return TMAT_OK;
}

// Test-only (tests/test_gpu_sep_quads_pool.py): ONE pooled fused separable launch in quadrant form and the full-frame quadrant fix-up
// behind it on host buffers with the caller's quadrant list (as tmat_debug_sepconv_quads).  x (n, hh, ww, cin); resid and out
// (n, hh / 2, ww / 2, cout).  The caller fills out: pooled pixels of quadrants not listed that are no boundary pixels of their quadrant
// (row or column 3 of its 4 x 4) come back as they went in; the fix-up pass rewrites every boundary pixel.
int tmat_debug_sepconv_pool_quads(tmat_handle hd, const float *x, int n, int hh, int ww, int cin, int relu_in, const float *dw9, const float *pw, int cout,
                                  const float *scale, const float *shift, int relu_out, const float *resid, const int *quads, int n_quads, float *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !x || !dw9 || !pw || !scale || !shift || !resid || !quads || !out || n < 1 || n_quads < 1 || n_quads > (1 << 24) || hh < 16 || ww < 16 ||
        cin < 1 || cout < 4 || ((cout / 4) & (cout / 4 - 1)) || !sepconv_ws_supported(hh, ww, cin, cout) ||
        (long long)n * hh * ww * std::max(cin, cout) > 0x3fffffffLL) {
        set_error("tmat_debug_sepconv_pool_quads: bad argument");
        return TMAT_E_ARG;
    }
    const long long nq = (long long)n * (hh / 8) * (ww / 8);
    std::vector<int> ids(quads, quads + n_quads);
    for (int id : ids) if (id < 0 || id >= nq) { set_error("tmat_debug_sepconv_pool_quads: a quadrant id lies outside the tensor"); return TMAT_E_ARG; }
    while (ids.size() % 4) ids.push_back(ids.back());
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    const size_t nx = (size_t)n * hh * ww * cin, no = (size_t)n * (hh / 2) * (ww / 2) * cout;
    std::vector<float> wk = k_contiguous(pw, 1, cin, cout);
    const size_t nw = wk.size();
    const float *hw = mem.keep(std::move(wk));
    const size_t n_ids = ids.size();
    const int *hid = mem.keep(std::move(ids));
    float *dx = mem.alloc_from(x, nx), *dd = mem.alloc_from(dw9, (size_t)9 * cin), *dw = mem.alloc_from(hw, nw);
    float *dsc = mem.alloc_from(scale, cout), *dsh = mem.alloc_from(shift, cout), *dres = mem.alloc_from(resid, no);
    float *dout = mem.alloc_from((const float *)out, no);
    float *strips = mem.alloc<float>(sepconv_pool_scratch_floats(n, hh, ww, cout, true));
    int *dq = mem.alloc_from(hid, n_ids);
    if (!mem.ok) return TMAT_E_HIP;
    if (!launch_sepconv_pool_ws(dx, n, hh, ww, cin, relu_in != 0, dd, dw, cout, dsc, dsh, relu_out != 0, strips, dres, dout, s, 0, nullptr, dq,
                                (int)(n_ids / 4), true)) return TMAT_E_ARG;
    mem.check(hipGetLastError(), "tmat_debug_sepconv_pool_quads launch");
    mem.d2h(out, dout, no * sizeof(float));
    if (mem.finish()) return TMAT_E_HIP;
    return TMAT_OK;
}

int tmat_debug_down_segs(tmat_handle h, int *max_segs)
{
    Ctx *c = (Ctx *)h;
    if (!c || !max_segs) { set_error("tmat_debug_down_segs: bad argument"); return TMAT_E_ARG; }
    *max_segs = c->down_segs;
    return TMAT_OK;
}

int tmat_debug_down_seg_total(tmat_handle h, int *total)
{
    Ctx *c = (Ctx *)h;
    if (!c || !total) { set_error("tmat_debug_down_seg_total: bad argument"); return TMAT_E_ARG; }
    *total = c->down_seg_total;
    return TMAT_OK;
}

// Stage-wise test entry point of the REGION form (tests/test_gpu_conv_roi.py): ONE launch_conv with a segment table on host buffers.
// The caller fills out (and out_relu): words outside the segments' rectangles come back as they went in.  nseg == 0: the full-frame launch
// of the same convolution.
static int conv2d_roi_impl(tmat_handle hd, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int stride, int subpixel, int cout,
                           const float *scale, const float *shift, const float *resid, int rs, int relu_in, int relu_out, const int *segs, int nseg,
                           float *out, float *out_relu, bool narrow = false)
{
    Ctx *c = (Ctx *)hd;
    const std::string who = narrow ? "tmat_conv2d_narrow" : "tmat_conv2d_roi";
    if (!c || !x || !w || !shift || !out || n < 1 || hh < 1 || ww < 1 || cin < 1 || cout < 1 || (ksize != 1 && ksize != 3) || (subpixel && ksize != 3) ||
        (subpixel && (resid || out_relu)) || (rs != 0 && rs != 1) || (rs && ((hh | ww) & 1)) || nseg < 0 || nseg > ROI_MAX_SEGS || (nseg && !segs) ||
        (stride != 1 && (stride != 2 || ksize != 1 || subpixel || resid || ((hh | ww) & 1)))) {
        set_error(who + ": bad argument (ksize 1 or 3, sub-pixel form of a 3x3 without residual or activated copy, rs 0 or 1, stride 2 with the "
                  "1x1 form without residual on even sides only, at most 64 segments)");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int up = subpixel ? 2 : 1;
    const size_t nx = (size_t)n * hh * ww * cin, no = (size_t)n * (hh * up / stride) * (ww * up / stride) * cout, nr = (size_t)n * (hh >> rs) * (ww >> rs) * cout;
    DevScope mem(c->ws_pool, s);
    // the weights as the network's own packing makes them (build_model): taps k-contiguous, the sub-pixel form pre-summed per parity class
    std::vector<float> wk = subpixel ? k_contiguous(subpixel_weights(std::vector<float>(w, w + (size_t)9 * cin * cout), cin, cout).data(), 16, cin, cout)
                                     : k_contiguous(w, ksize * ksize, cin, cout);
    const size_t nw = wk.size();
    const float *hw = mem.keep(std::move(wk));
    float *dx = mem.alloc_from(x, nx), *dw = mem.alloc_from(hw, nw);
    float *dsh = mem.alloc_from(shift, cout), *dsc = scale ? mem.alloc_from(scale, cout) : nullptr;
    float *dr = resid ? mem.alloc_from(resid, nr) : nullptr, *dout = mem.alloc_from((const float *)out, no);
    float *dout2 = out_relu ? mem.alloc_from((const float *)out_relu, no) : nullptr;
    if (!mem.ok) return TMAT_E_HIP;
    ConvArgs a{};
    a.in = dx; a.N = n; a.h = hh; a.w = ww; a.Cin = cin; a.relu_in = relu_in != 0; a.ksize = subpixel ? 2 : ksize; a.stride = stride; a.W = dw;
    a.Cout = cout; a.scale = dsc; a.shift = dsh; a.resid = dr; a.rs = rs; a.relu_out = relu_out != 0; a.out = dout; a.out_relu = dout2; a.prec = 0;
    RoiSegs sg{};
    for (int i = 0; i < nseg; i++) {
        RoiSeg &g = sg.s[sg.nseg++];
        g.p0 = segs[6 * i]; g.np = segs[6 * i + 1]; g.y0 = segs[6 * i + 2]; g.x0 = segs[6 * i + 3]; g.rh = segs[6 * i + 4]; g.rw = segs[6 * i + 5];
    }
    if (!(narrow ? launch_conv_narrow(a, s, nseg ? &sg : nullptr) : launch_conv(a, s, nseg ? &sg : nullptr))) return TMAT_E_ARG;
    mem.check(hipGetLastError(), narrow ? "tmat_conv2d_narrow launch" : "tmat_conv2d_roi launch");
    mem.d2h(out, dout, no * sizeof(float));
    if (out_relu) mem.d2h(out_relu, dout2, no * sizeof(float));
    if (mem.finish()) return TMAT_E_HIP;
    return TMAT_OK;
}

int tmat_conv2d_roi(tmat_handle hd, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int subpixel, int cout,
                    const float *scale, const float *shift, const float *resid, int rs, int relu_in, int relu_out, const int *segs, int nseg,
                    float *out, float *out_relu)
{
    return conv2d_roi_impl(hd, x, n, hh, ww, cin, w, ksize, 1, subpixel, cout, scale, shift, resid, rs, relu_in, relu_out, segs, nseg, out, out_relu);
}

// the 1x1 form at stride 2 (the down path's residual launches): out (n, hh / 2, ww / 2, cout), the segments' rectangles are output pixels
int tmat_conv2d_roi_s2(tmat_handle hd, const float *x, int n, int hh, int ww, int cin, const float *w, int cout, const float *scale,
                       const float *shift, int relu_in, int relu_out, const int *segs, int nseg, float *out, float *out_relu)
{
    return conv2d_roi_impl(hd, x, n, hh, ww, cin, w, 1, 2, 0, cout, scale, shift, nullptr, 0, relu_in, relu_out, segs, nseg, out, out_relu);
}

// The same entry point on the narrow layers' kernel (conv_narrow_kernels.hip; tests/test_gpu_conv_narrow.py): ONE launch_conv_narrow
int tmat_conv2d_narrow(tmat_handle hd, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int stride, int subpixel, int cout,
                       const float *scale, const float *shift, const float *resid, int rs, int relu_in, int relu_out, const int *segs, int nseg,
                       float *out, float *out_relu)
{
    return conv2d_roi_impl(hd, x, n, hh, ww, cin, w, ksize, stride, subpixel, cout, scale, shift, resid, rs, relu_in, relu_out, segs, nseg, out, out_relu, true);
}

int tmat_model_layers(const void *blob, size_t n_bytes, int cap, int *layers, int *n_layers)
{
    if (!blob || !n_layers || cap < 0 || (cap > 0 && !layers)) { set_error("tmat_model_layers: bad argument"); return TMAT_E_ARG; }
    *n_layers = 0;
    std::map<std::string, Tensor> m;
    int patch = 0;
    ModelShape ms;
    std::vector<ModelLayer> ls;
    if (!parse_blob(blob, n_bytes, m, patch) || !model_shape(m, patch, ms) || !model_layers(ms, unet_switches_from_env(), ls)) return TMAT_E_WEIGHTS;
    *n_layers = (int)ls.size();
    if (*n_layers > cap) { set_error("tmat_model_layers: cap is below the number of launches (n_layers holds it)"); return TMAT_E_CAP; }
    for (size_t i = 0; i < ls.size(); i++) {
        const int v[6] = {ls[i].ksize, ls[i].stride, ls[i].cin, ls[i].cout, ls[i].side, ls[i].launcher};
        memcpy(layers + 6 * i, v, sizeof(v));
    }
    return TMAT_OK;
}

int tmat_prof_enable(tmat_handle h, int on)
{
    Ctx *c = (Ctx *)h;
    if (!c) { set_error("null handle"); return TMAT_E_ARG; }
    c->prof_on = on != 0;
    return TMAT_OK;
}
int tmat_prof_read(tmat_handle h, double *ms, int64_t *launches, double *flops, int reset)
{
    Ctx *c = (Ctx *)h;
    if (!c) { set_error("null handle"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    TMAT_HIP(hipStreamSynchronize(c->stream));
    for (auto &e : c->ev_open) {
        float t = 0;
        if (hipEventElapsedTime(&t, e.e0, e.e1) == hipSuccess) { c->prof_ms += t; c->prof_launches++; c->prof_flops += e.flops; }
        c->ev_pool.push_back(e.e0); c->ev_pool.push_back(e.e1);
    }
    c->ev_open.clear();
    if (ms) *ms = c->prof_ms;
    if (launches) *launches = c->prof_launches;
    if (flops) *flops = c->prof_flops;
    if (reset) { c->prof_ms = 0; c->prof_launches = 0; c->prof_flops = 0; }
    return TMAT_OK;
}

// ---- PNG encoder (png.h) ----

int tmat_png_stripe(void) { return PNG_STRIPE; }

int tmat_png_bound(int H, int W, int channels, size_t *bound)
{
    PngShape g;
    if (!bound || !png_shape(H, W, channels, g)) { set_error("tmat_png_bound: bad argument (H, W >= 1, channels 1 or 3, below 2^31 bytes)"); return TMAT_E_ARG; }
    *bound = g.bound;
    return TMAT_OK;
}

static int png_args(const char *who, const void *pics, int n, int H, int W, int channels, const void *out, size_t cap_each, const size_t *sizes, PngShape &g)
{
    if (n < 0 || !png_shape(H, W, channels, g) || (n && (!pics || !out || !sizes))) {
        set_error(std::string(who) + ": bad argument (H, W >= 1, channels 1 or 3, below 2^31 bytes)");
        return TMAT_E_ARG;
    }
    if (cap_each < g.bound) { set_error(std::string(who) + ": cap_each is below tmat_png_bound"); return TMAT_E_CAP; }
    return TMAT_OK;
}

int tmat_host_png_encode_batch(const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes)
{
    PngShape g;
    if (int rc = png_args("tmat_host_png_encode_batch", pics, n, H, W, channels, out, cap_each, sizes, g)) return rc;
    for (int i = 0; i < n; i++) png_encode_host(pics + (size_t)i * H * g.rb, g, PNG_FAST, out + (size_t)i * cap_each, &sizes[i]);
    return TMAT_OK;
}

int tmat_host_png_encode_batch_mode(const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes, int mode)
{
    PngShape g;
    if (mode != TMAT_PNG_FAST && mode != TMAT_PNG_COMPACT) { set_error("tmat_host_png_encode_batch_mode: mode must be TMAT_PNG_FAST or TMAT_PNG_COMPACT"); return TMAT_E_ARG; }
    if (int rc = png_args("tmat_host_png_encode_batch_mode", pics, n, H, W, channels, out, cap_each, sizes, g)) return rc;
    for (int i = 0; i < n; i++) png_encode_host(pics + (size_t)i * H * g.rb, g, mode, out + (size_t)i * cap_each, &sizes[i]);
    return TMAT_OK;
}

int tmat_png_set_mode(tmat_handle h, int mode)
{
    Ctx *c = (Ctx *)h;
    if (!c || (mode != TMAT_PNG_FAST && mode != TMAT_PNG_COMPACT)) { set_error("tmat_png_set_mode: needs a handle and mode TMAT_PNG_FAST or TMAT_PNG_COMPACT"); return TMAT_E_ARG; }
    c->png_mode = mode;
    return TMAT_OK;
}

// the contract of png_code_lengths (png.h)
static bool png_code_lengths_args(const uint32_t *freq, size_t k, int n, int limit, const uint8_t *len)
{
    if (!freq || !len || n < 1 || n > PNG_NLL || limit < 1 || limit > 15 || (1 << limit) < n) return false;
    for (size_t i = 0; i < k; i++) {
        uint64_t sum = 0;
        for (int j = 0; j < n; j++) sum += freq[i * n + j];
        if (sum >= (1u << 22)) return false;
    }
    return true;
}

int tmat_host_png_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len)
{
    if (!png_code_lengths_args(freq, 1, n, limit, len)) { set_error("tmat_host_png_code_lengths: bad argument (1 <= n <= 286, 2^limit >= n, limit <= 15, sum of frequencies below 2^22)"); return TMAT_E_ARG; }
    png_code_lengths(freq, n, limit, len);
    return TMAT_OK;
}

int tmat_debug_png_code_lengths(tmat_handle h, const uint32_t *freqs, int k, int n, int limit, uint8_t *lens)
{
    Ctx *c = (Ctx *)h;
    if (!c || k < 0 || (k && !png_code_lengths_args(freqs, (size_t)k, n, limit, lens))) {
        set_error("tmat_debug_png_code_lengths: bad argument (a handle, 1 <= n <= 286, 2^limit >= n, limit <= 15, sums of frequencies below 2^22)");
        return TMAT_E_ARG;
    }
    if (k == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    DevScope mem(c->ws_pool, c->stream);
    uint32_t *df = mem.pooled<uint32_t>((size_t)k * n);
    uint8_t *dl = mem.pooled<uint8_t>((size_t)k * n);
    if (!mem.ok) return TMAT_E_HIP;
    mem.h2d(df, freqs, (size_t)k * n * sizeof(uint32_t));
    if (!mem.ok) return TMAT_E_HIP;
    if (png_code_lengths_launch(df, k, n, limit, dl, c->stream)) { set_error("tmat_debug_png_code_lengths: kernel launch failed"); return TMAT_E_HIP; }
    mem.d2h(lens, dl, (size_t)k * n);
    return mem.finish() ? TMAT_E_HIP : TMAT_OK;
}

static int png_encode_api(const char *who, tmat_handle hd, const uint8_t *pics, bool on_host, int n, int H, int W, int channels, uint8_t *out,
                          size_t cap_each, size_t *sizes, float *ms3)
{
    Ctx *c = (Ctx *)hd;
    PngShape g;
    if (!c) { set_error(std::string(who) + ": null handle"); return TMAT_E_ARG; }
    if (int rc = png_args(who, pics, n, H, W, channels, out, cap_each, sizes, g)) return rc;
    if (ms3) ms3[0] = ms3[1] = ms3[2] = 0.0f;
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    return png_encode_ctx(c, pics, on_host, n, g, out, cap_each, sizes, ms3);
}

int tmat_png_encode_batch(tmat_handle h, const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes)
{
    return png_encode_api("tmat_png_encode_batch", h, pics, true, n, H, W, channels, out, cap_each, sizes, nullptr);
}
int tmat_png_encode_batch_dev(tmat_handle h, const uint8_t *pics_dev, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes)
{
    return png_encode_api("tmat_png_encode_batch_dev", h, pics_dev, false, n, H, W, channels, out, cap_each, sizes, nullptr);
}
int tmat_png_encode_batch_timed(tmat_handle h, const uint8_t *pics, int n, int H, int W, int channels, uint8_t *out, size_t cap_each, size_t *sizes,
                                float *ms3)
{
    if (!ms3) { set_error("tmat_png_encode_batch_timed: bad argument"); return TMAT_E_ARG; }
    return png_encode_api("tmat_png_encode_batch_timed", h, pics, true, n, H, W, channels, out, cap_each, sizes, ms3);
}

// ---- TIFF decoder (tiff.h) ----

int tmat_tiff_probe(const uint8_t *file, size_t n_bytes, int cap_pages, tmat_tiff_page *pages, int *n_pages)
{
    static_assert(sizeof(tmat_tiff_page) == sizeof(TiffPageInfo), "tmat_tiff_page and TiffPageInfo are one layout");
    if (!file || !n_pages || cap_pages < 0 || (cap_pages > 0 && !pages)) { set_error("tmat_tiff_probe: bad argument"); return TMAT_E_ARG; }
    tiff_walk(file, n_bytes, cap_pages, (TiffPageInfo *)pages, n_pages, -1, nullptr);
    return TMAT_OK;
}

static int tiff_args(const char *who, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of, int n_planes,
                     int H, int W, const void *out, int *bits, int *status, TiffPlan &plan)
{
    bool ok = n_planes >= 0 && H >= 1 && W >= 1 && bits && (n_planes == 0 || (files && n_bytes && file_of && page_of && out && status));
    ok = ok && (uint64_t)H * (uint64_t)W * 2 <= TIFF_MAX_PLANE_BYTES;
    for (int i = 0; ok && i < n_planes; i++) ok = file_of[i] >= 0 && page_of[i] >= 0 && page_of[i] < (1 << 20);
    if (!ok) { set_error(std::string(who) + ": bad argument (planes of one shape H, W >= 1 of at most 2^30 bytes, pages below 2^20)"); return TMAT_E_ARG; }
    std::string err;
    if (!tiff_plan(files, n_bytes, file_of, page_of, n_planes, H, W, plan, status, err)) { set_error(std::string(who) + ": " + err); return TMAT_E_ARG; }
    *bits = plan.bits;
    return TMAT_OK;
}

int tmat_host_tiff_decode_batch(const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of, int n_planes,
                                int H, int W, uint16_t *out, int *bits, int *status)
{
    TiffPlan plan;
    if (int rc = tiff_args("tmat_host_tiff_decode_batch", files, n_bytes, file_of, page_of, n_planes, H, W, out, bits, status, plan)) return rc;
    tiff_decode_host(files, file_of, plan, H, W, out, status);
    return TMAT_OK;
}

static int tiff_decode_api(const char *who, tmat_handle hd, const uint8_t *const *files, const size_t *n_bytes, const int *file_of,
                           const int *page_of, int n_planes, int H, int W, void *out, bool out_on_host, int *bits, int *status, float *ms2 = nullptr)
{
    Ctx *c = (Ctx *)hd;
    if (!c) { set_error(std::string(who) + ": null handle"); return TMAT_E_ARG; }
    TiffPlan plan;
    if (int rc = tiff_args(who, files, n_bytes, file_of, page_of, n_planes, H, W, out, bits, status, plan)) return rc;
    if (ms2) ms2[0] = ms2[1] = 0.0f;
    if (n_planes == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    return tiff_decode_ctx(c, files, n_bytes, file_of, plan, H, W, (uint16_t *)out, out_on_host, status, ms2);
}

int tmat_tiff_decode_batch(tmat_handle h, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of,
                           int n_planes, int H, int W, uint16_t *out_host, int *bits, int *status)
{
    return tiff_decode_api("tmat_tiff_decode_batch", h, files, n_bytes, file_of, page_of, n_planes, H, W, out_host, true, bits, status);
}
int tmat_tiff_decode_batch_dev(tmat_handle h, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of,
                               int n_planes, int H, int W, void *out_dev, int *bits, int *status)
{
    return tiff_decode_api("tmat_tiff_decode_batch_dev", h, files, n_bytes, file_of, page_of, n_planes, H, W, out_dev, false, bits, status);
}
int tmat_tiff_decode_batch_dev_timed(tmat_handle h, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of,
                                     int n_planes, int H, int W, void *out_dev, int *bits, int *status, float *ms2)
{
    if (!ms2) { set_error("tmat_tiff_decode_batch_dev_timed: bad argument"); return TMAT_E_ARG; }
    return tiff_decode_api("tmat_tiff_decode_batch_dev_timed", h, files, n_bytes, file_of, page_of, n_planes, H, W, out_dev, false, bits, status, ms2);
}

}  // extern "C"

namespace tmat {

int png_encode_ctx(Ctx *c, const uint8_t *pics, bool on_host, int n, const PngShape &g, uint8_t *out, size_t cap_each, size_t *sizes, float *ms3)
{
    hipStream_t s = c->stream;
    const size_t pic_bytes = (size_t)g.H * g.rb, fcap = (g.bound + 15) & ~(size_t)15;
    const int K = (int)std::max<size_t>(1, std::min<size_t>(std::min(n, 65535), ((size_t)128 << 20) / g.raw));     // <= 128 MiB of filtered stream per chunk
    struct Events { hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); } } ev;
    DevScope mem(c->ws_pool, s);        // after ev: the events go when the stream has drained
    if (ms3) for (hipEvent_t &e : ev.e) mem.check(hipEventCreate(&e), "hipEventCreate");
    auto mark = [&](int i) { if (ms3 && mem.ok) mem.check(hipEventRecord(ev.e[i], s), "hipEventRecord"); };
    auto span = [&](int a, int b, int slot) { float t = 0.0f; if (ms3 && hipEventElapsedTime(&t, ev.e[a], ev.e[b]) == hipSuccess) ms3[slot] += t; };
    uint8_t *dpic = on_host ? mem.pooled<uint8_t>((size_t)K * pic_bytes) : nullptr;
    uint8_t *filt = mem.pooled<uint8_t>((size_t)K * g.raw), *slots = mem.pooled<uint8_t>((size_t)K * g.ns * PNG_SLOT);
    uint8_t *files = mem.pooled<uint8_t>((size_t)K * fcap);
    uint32_t *meta = mem.pooled<uint32_t>((size_t)K * g.ns * 4), *dsz = mem.pooled<uint32_t>(K);
    uint32_t *hsz = mem.host<uint32_t>(K);
    if (!mem.ok) return TMAT_E_HIP;
    for (int i0 = 0; i0 < n; i0 += K) {
        const int k = std::min(K, n - i0);
        const uint8_t *src = pics + (size_t)i0 * pic_bytes;
        mark(0);
        if (on_host) { mem.h2d(dpic, src, (size_t)k * pic_bytes); src = dpic; }
        mark(1);
        if (!mem.ok) return TMAT_E_HIP;
        if (png_encode_launch(src, k, g, c->png_mode, filt, slots, meta, files, fcap, dsz, s)) { set_error("png encoder: kernel launch failed"); return TMAT_E_HIP; }
        mark(2);
        mem.d2h(hsz, dsz, (size_t)k * sizeof(uint32_t));
        if (mem.finish()) return TMAT_E_HIP;
        for (int i = 0; i < k; i++) {
            if (hsz[i] < PNG_HEAD + PNG_TAIL || hsz[i] > g.bound) { set_error("png encoder: a file left its bound"); return TMAT_E_HIP; }
            mem.d2h(out + (size_t)(i0 + i) * cap_each, files + (size_t)i * fcap, hsz[i]);
            sizes[i0 + i] = hsz[i];
        }
        mark(3);
        if (mem.finish()) return TMAT_E_HIP;
        span(0, 1, 0); span(1, 2, 1); span(2, 3, 2);
    }
    return TMAT_OK;
}

// pool requests of the decoder in a few sizes per magnitude, so that calls of different batches share the pool's blocks
static size_t tiff_pool_size(size_t bytes)
{
    size_t step = 4096;
    while (step * 8 < bytes) step *= 2;
    return (bytes + step - 1) / step * step;
}

// The planes of `plan` in chunks of consecutive planes: at most TIFF_CHUNK_BYTES of file bytes, of raw strip bytes and (out_on_host) of
// pixels per chunk -- one plane at least -- each file uploaded once per chunk, whole.
int tiff_decode_ctx(Ctx *c, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const TiffPlan &plan, int H, int W,
                    uint16_t *out, bool out_on_host, int *status, float *ms2)
{
    constexpr size_t TIFF_CHUNK_BYTES = (size_t)256 << 20;
    hipStream_t s = c->stream;
    const size_t n = plan.planes.size(), px = (size_t)H * W;
    struct Events { hipEvent_t e[3] = {nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); } } ev;
    if (ms2) for (hipEvent_t &e : ev.e) TMAT_HIP(hipEventCreate(&e));
    for (size_t i0 = 0; i0 < n;) {
        // the chunk [i0, i1): its files, strips and planes with chunk-relative indices
        std::map<int, uint64_t> base;           // file -> first byte in the blob
        std::vector<TiffPlane> planes;
        std::vector<TiffStrip> strips;
        size_t blob_bytes = 0, raw_bytes = 0, i1 = i0;
        for (; i1 < n && i1 - i0 < 65535; i1++) {
            TiffPlane p = plan.planes[i1];
            size_t add_blob = 0, add_raw = 0;
            if (p.ok) {
                if (!base.count(file_of[i1])) add_blob = (n_bytes[file_of[i1]] + 15) & ~(size_t)15;
                if (p.comp != TIFF_COMP_NONE) add_raw = (px * (size_t)p.bytes + 15) & ~(size_t)15;
                if (i1 > i0 && (blob_bytes + add_blob > TIFF_CHUNK_BYTES || raw_bytes + add_raw > TIFF_CHUNK_BYTES ||
                                (out_on_host && (i1 - i0 + 1) * px * 2 > TIFF_CHUNK_BYTES))) break;
                if (add_blob) { base[file_of[i1]] = blob_bytes; blob_bytes += add_blob; }
                p.file_base = base[file_of[i1]];
                p.raw = raw_bytes;
                raw_bytes += add_raw;
                const int ns = (H + p.rps - 1) / p.rps, first = (int)strips.size();
                for (int k = 0; k < ns; k++) {
                    TiffStrip st = plan.strips[(size_t)p.first_strip + k];
                    st.plane = (int32_t)(i1 - i0);
                    strips.push_back(st);
                }
                p.first_strip = first;
            }
            p.out_index = (int32_t)(out_on_host ? i1 - i0 : i1);
            planes.push_back(p);
        }
        const size_t k = i1 - i0;
        if (!strips.empty()) {
            DevScope mem(c->ws_pool, s);
            uint8_t *blob = (uint8_t *)mem.pooled_bytes(tiff_pool_size(blob_bytes));
            uint8_t *raw = (uint8_t *)mem.pooled_bytes(tiff_pool_size(std::max<size_t>(raw_bytes, 16)));
            uint16_t *dout = out_on_host ? (uint16_t *)mem.pooled_bytes(tiff_pool_size(k * px * 2)) : out;
            TiffStrip *dstrips = (TiffStrip *)mem.pooled_bytes(tiff_pool_size(strips.size() * sizeof(TiffStrip)));
            TiffPlane *dplanes = (TiffPlane *)mem.pooled_bytes(tiff_pool_size(k * sizeof(TiffPlane)));
            int *dbad = (int *)mem.pooled_bytes(tiff_pool_size(k * sizeof(int)));
            int *hbad = mem.host<int>(k);
            if (!mem.ok) return TMAT_E_HIP;
            auto mark = [&](int i) { if (ms2 && mem.ok) mem.check(hipEventRecord(ev.e[i], s), "hipEventRecord"); };
            mark(0);
            for (auto &fb : base) mem.h2d(blob + fb.second, files[fb.first], n_bytes[fb.first]);
            mem.h2d(dstrips, strips.data(), strips.size() * sizeof(TiffStrip));
            mem.h2d(dplanes, planes.data(), k * sizeof(TiffPlane));
            mark(1);
            if (!mem.ok) return TMAT_E_HIP;
            if (tiff_decode_launch(blob, dstrips, (int)strips.size(), dplanes, (int)k, H, W, raw, dout, dbad, s)) {
                set_error("tiff decoder: kernel launch failed");
                return TMAT_E_HIP;
            }
            mark(2);
            mem.d2h(hbad, dbad, k * sizeof(int));
            if (mem.finish()) return TMAT_E_HIP;           // strips and planes are host temporaries of this turn: drained before they go
            for (int a = 0; ms2 && a < 2; a++) { float t = 0.0f; if (hipEventElapsedTime(&t, ev.e[a], ev.e[a + 1]) == hipSuccess) ms2[a] += t; }
            for (size_t j = 0; j < k; j++) {
                if (!planes[j].ok) continue;
                if (hbad[j]) status[i0 + j] = TIFF_CORRUPT;
                else if (out_on_host) mem.d2h(out + (i0 + j) * px, dout + j * px, px * 2);
            }
            if (mem.finish()) return TMAT_E_HIP;
        }
        i0 = i1;
    }
    return TMAT_OK;
}

}  // namespace tmat
