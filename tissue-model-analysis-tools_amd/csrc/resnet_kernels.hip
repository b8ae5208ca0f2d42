// Invasion-depth tool on gfx950 (reference scripts/compute_inv_depth.py:96-172, fl_tissue_model_tools/models.py:33-82,
// data_prep.py:17-61): per Z slice a ResNet50 trunk up to conv4_block6_out (keras.applications.resnet50), global average
// pooling, one dense unit, sigmoid; an ensemble of such models votes by the mean probability.
//
// The trunk is 1x1 and 3x3 convolutions with folded BatchNormalization: they run on the f32-MFMA implicit-GEMM kernel of the
// branching path (unet_kernels.hip: conv_mfma_kernel, 1x1 stride 1 / 2, 3x3 SAME, residual add + ReLU in the epilogue), so the
// two tools share their hot kernel and its arithmetic contract (oracle/unet_exact.c:orc_conv).  New here: the data
// preparation (bilinear resize, rescale to 0..255, caffe-style mean subtraction), the 7x7 stride-2 stem, the 3x3 stride-2
// max-pool and the head.  Keras details: every Conv2D has a bias, BatchNormalization eps = 1.001e-5, ZeroPadding2D(3) before
// the stem convolution and ZeroPadding2D(1) before the pool (both 'valid'), the stride of a stage sits in the first 1x1
// convolution of its first block and in that block's projection shortcut.
// The 7x7 stride-2 stem runs on the same MFMA kernel (round 4): resnet_im2col_kernel lays the 147 taps of every output pixel out as
// a 192-channel pixel (k = (ky 7 + kx) 3 + c, zeros outside the image and for k >= 147: six K chunks of 32) and the convolution
// becomes a 1x1 layer with K = 192; round 3's direct kernel (one thread per output, 147 LDS + 147 cached global reads each) took
// 18 % of the tool's GPU time at 12 TFLOP/s.
// Arithmetic of the new kernels (shared with oracle/resnet.py): float32, multiply and add kept separate (no FMA) in pool and
// head; stem: orc_conv's chain over k (the MFMA order) on the im2col tensor, fmaf(acc, scale, shift), ReLU; head: per channel sum over the 256 pixels in raster order, times 1/256, dot product over
// the channels in order, plus bias, 1 / (1 + exp_det(-z)).
// Opt-in modes (tmat_resnet_set_precision): f16 -- the convolutions on conv_mfma_kernel's PREC = 3 form, activations f32 in memory;
// f16act -- every activation tensor IEEE binary16 in memory: conv_f16act_kernels.hip, resnet_im2col_f16_kernel and the _Float16 forms of
// the pool and head kernels below, in the first half of the same buffers (resnet_forward_f16act_dev).
#include "../../include/tmat.h"
#include "tmat_ctx.h"

#include <cmath>
#include <cstring>

namespace tmat {

// (N, S, S) u16 slices (already resized) -> (N, S, S, 3) f32: rescale_intensity(img, (0, 255)) in f64 (per image), the three
// identical channels minus the caffe means of B, G, R (resnet50.preprocess_input), cast to f32 (tf.convert_to_tensor)
__global__ __launch_bounds__(256) void inv_prep_kernel(const uint16_t *__restrict__ img, int npx, const int *__restrict__ mn, const int *__restrict__ mx,
                                                       float *__restrict__ out)
{
    const int n = blockIdx.y;
    const double lo = (double)mn[n], hi = (double)mx[n];
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npx; p += gridDim.x * 256) {
        const double x = (double)img[(size_t)n * npx + p];
        double g = fmin(fmax(x, lo), hi);
        g = lo != hi ? ((g - lo) / (hi - lo)) * 255.0 + 0.0 : fmin(fmax(g, 0.0), 255.0);
        float *o = out + ((size_t)n * npx + p) * 3;
        o[0] = (float)(g - 103.939); o[1] = (float)(g - 116.779); o[2] = (float)(g - 123.68);
    }
}
__global__ __launch_bounds__(256) void minmax_u16_img_kernel(const uint16_t *__restrict__ img, int npx, int *__restrict__ mn, int *__restrict__ mx)
{
    const uint16_t *p = img + (size_t)blockIdx.x * npx;
    int lo = 65535, hi = 0;
    for (int i = threadIdx.x; i < npx; i += 256) { const int v = p[i]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    for (int o = 32; o > 0; o >>= 1) { const int l2 = __shfl_down(lo, o), h2 = __shfl_down(hi, o); lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; }
    __shared__ int sl[4], sh[4];
    if ((threadIdx.x & 63) == 0) { sl[threadIdx.x >> 6] = lo; sh[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; i++) { lo = sl[i] < lo ? sl[i] : lo; hi = sh[i] > hi ? sh[i] : hi; }
        mn[blockIdx.x] = lo; mx[blockIdx.x] = hi;
    }
}

// conv1: ZeroPadding2D(3) + Conv2D(64, 7, strides 2, valid) + BN + ReLU, as im2col + a 1x1 convolution on conv_mfma_kernel.
// x (N, S, S, 3) -> col (N, S/2, S/2, 192): col[k] = x[2 yo + ky - 3][2 xo + kx - 3][c] for k = (ky 7 + kx) 3 + c < 147 (0 outside the
// image: the zero padding), 0 for 147 <= k < 192.  One thread = 4 consecutive k of one output pixel (one 16-byte store).
constexpr int STEM_TAPS = 147, STEM_K = 192;
__global__ __launch_bounds__(256) void resnet_im2col_kernel(const float *__restrict__ x, int S, float *__restrict__ col, size_t total)
{
    const int So = S >> 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int q = (int)(e % (STEM_K / 4));
        const size_t pix = e / (STEM_K / 4);
        const int xo = (int)(pix % So), yo = (int)((pix / So) % So);
        const size_t n = pix / ((size_t)So * So);
        const float *xi = x + n * S * S * 3;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = 4 * q + j;
            const int tap = k / 3, c = k - tap * 3;
            const int ky = tap / 7, kx = tap - ky * 7;
            const int iy = 2 * yo + ky - 3, ix = 2 * xo + kx - 3;
            const bool in = k < STEM_TAPS && iy >= 0 && iy < S && ix >= 0 && ix < S;
            v[j] = in ? xi[((size_t)iy * S + ix) * 3 + c] : 0.0f;
        }
        *reinterpret_cast<float4 *>(col + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// the f16act form: the same tensor as IEEE binary16 -- THE one rounding of the prepared input (nearest even, magnitudes above
// 65504 saturating).  One thread = 8 consecutive k of one output pixel (one 16-byte store).
typedef _Float16 f16x8_r __attribute__((ext_vector_type(8)));
__device__ __forceinline__ _Float16 f16_sat_r(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }
__global__ __launch_bounds__(256) void resnet_im2col_f16_kernel(const float *__restrict__ x, int S, _Float16 *__restrict__ col, size_t total)
{
    const int So = S >> 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int q = (int)(e % (STEM_K / 8));
        const size_t pix = e / (STEM_K / 8);
        const int xo = (int)(pix % So), yo = (int)((pix / So) % So);
        const size_t n = pix / ((size_t)So * So);
        const float *xi = x + n * S * S * 3;
        f16x8_r v;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = 8 * q + j;
            const int tap = k / 3, c = k - tap * 3;
            const int ky = tap / 7, kx = tap - ky * 7;
            const int iy = 2 * yo + ky - 3, ix = 2 * xo + kx - 3;
            const bool in = k < STEM_TAPS && iy >= 0 && iy < S && ix >= 0 && ix < S;
            v[j] = f16_sat_r(in ? xi[((size_t)iy * S + ix) * 3 + c] : 0.0f);
        }
        *reinterpret_cast<f16x8_r *>(col + e * 8) = v;
    }
}

// pool1: ZeroPadding2D(1) + MaxPooling2D(3, strides 2, valid): (N, S, S, C) -> (N, S/2, S/2, C); the padding is ZEROS
// T = float, or _Float16 (f16act: the maximum of f16 values is one of them: exact)
template <typename T>
__global__ __launch_bounds__(256) void resnet_pool_kernel(const T *__restrict__ x, int S, int C, T *__restrict__ out, size_t total)
{
    const int So = S >> 1;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C);
        const size_t q = e / C;
        const int xo = (int)(q % So), yo = (int)((q / So) % So);
        const size_t n = q / ((size_t)So * So);
        float m = -INFINITY;
        for (int ky = 0; ky < 3; ky++)
            for (int kx = 0; kx < 3; kx++) {
                const int iy = 2 * yo + ky - 1, ix = 2 * xo + kx - 1;
                const float v = (iy >= 0 && iy < S && ix >= 0 && ix < S) ? (float)x[((n * S + iy) * S + ix) * C + c] : 0.0f;
                m = v > m ? v : m;
            }
        out[e] = (T)m;
    }
}

__device__ __forceinline__ float exp_det_r(float x)        // the deterministic expf of unet_kernels.hip / oracle/unet_exact.c
{
    x = fminf(fmaxf(x, -88.0f), 88.0f);
    float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693359375f, x);
    r = fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    float r2 = r * r;
    float y = fmaf(p, r2, r) + 1.0f;
    return ldexpf(y, (int)n);
}

// GlobalAveragePooling2D + Dense(1) + sigmoid: feat (N, P, C) -> prob (N); one block per image, thread = channel (C <= 1024)
// T = float, or _Float16 (f16act: the features widened exactly, the arithmetic unchanged)
template <typename T>
__global__ __launch_bounds__(1024) void resnet_head_kernel(const T *__restrict__ feat, int P, int C, const float *__restrict__ w, float b, float *__restrict__ prob)
{
    __shared__ float sm[1024];
    const int c = threadIdx.x;
    if (c < C) {
        const T *f = feat + (size_t)blockIdx.x * P * C + c;
        float s = 0.0f;
        for (int p = 0; p < P; p++) s = s + (float)f[(size_t)p * C];
        sm[c] = s * (1.0f / (float)P);
    }
    __syncthreads();
    if (c == 0) {
        float z = 0.0f;
        for (int k = 0; k < C; k++) z = z + sm[k] * w[k];
        z = z + b;
        prob[blockIdx.x] = 1.0f / (1.0f + exp_det_r(-z));
    }
}

static bool up(ResNetModel &m, const std::vector<float> &v, float **dev)
{
    if (!hip_ok(hipMalloc((void **)dev, v.size() * sizeof(float)), "hipMalloc(resnet weights)")) return false;
    m.owned.push_back(*dev);
    return hip_ok(hipMemcpy(*dev, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(resnet weights)");
}
// scale = f32(gamma / sqrt(var + 1.001e-5)); shift = f32(beta + (bias - mean) * scale_f64)
static void fold_bn_keras(const Tensor &bn, const Tensor &bias, std::vector<float> &scale, std::vector<float> &shift)
{
    const int C = bn.shape[1];
    scale.resize(C); shift.resize(C);
    for (int i = 0; i < C; i++) {
        const double g = bn.data[i], b = bn.data[C + i], mu = bn.data[2 * C + i], v = bn.data[3 * C + i];
        const double sd = g / std::sqrt(v + 1.001e-5);
        scale[i] = (float)sd;
        shift[i] = (float)(b + ((double)bias.data[i] - mu) * sd);
    }
}
static bool load_conv(ResNetModel &m, const std::map<std::string, Tensor> &t, const std::string &name, int ksize, int stride, int cin_expect, ResConv &c)
{
    auto w = t.find(name + ".w"), b = t.find(name + ".b"), bn = t.find(name + ".bn");
    if (w == t.end() || b == t.end() || bn == t.end()) { set_error("resnet weights: missing " + name); return false; }
    const Tensor &W = w->second;
    if (W.shape.size() != 4 || W.shape[0] != ksize || W.shape[1] != ksize || W.shape[2] != cin_expect || W.shape[3] % 64 || cin_expect % 32) {
        set_error("resnet weights: bad shape of " + name + ".w");
        return false;
    }
    c.cin = W.shape[2]; c.cout = W.shape[3]; c.ksize = ksize; c.stride = stride;
    if (bn->second.shape.size() != 2 || bn->second.shape[0] != 4 || bn->second.shape[1] != c.cout || (int)b->second.count != c.cout) {
        set_error("resnet weights: BatchNormalization / bias of " + name + " does not match");
        return false;
    }
    std::vector<float> sc, sh;
    fold_bn_keras(bn->second, b->second, sc, sh);
    return up(m, k_contiguous(W.data, ksize * ksize, c.cin, c.cout), &c.w) && up(m, sc, &c.scale) && up(m, sh, &c.shift);
}

// IEEE binary16 bits of x: round to nearest even, magnitudes above 65504 saturate to +-65504 (never inf; no NaNs in weights), results
// below 2^-14 are f16 subnormals (kept as such: DESIGN 7c says what the matrix instruction does with them).
static uint16_t f16_rne_sat(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u >= 0x477fe000u) return sign | 0x7bffu;          // |x| >= 65504 (and inf / NaN): saturate
    float ax;
    memcpy(&ax, &u, 4);
    if (u < 0x38800000u) {                                  // |x| < 2^-14: subnormal f16, grid 2^-24
        // |x| 2^24 < 2^10 (exact) rounds to an integer, nearest even, in the addition of 2^23
        float r = ax * 16777216.0f + 8388608.0f;
        uint32_t ru;
        memcpy(&ru, &r, 4);
        return sign | (uint16_t)(ru - 0x4b000000u);         // 0 .. 1024 (1024 = the smallest normal)
    }
    // normal: keep 10 mantissa bits, nearest even on the 13 dropped ones (a carry into the exponent is the right answer)
    const uint32_t rounded = u + 0x00000fffu + ((u >> 13) & 1u);
    return sign | (uint16_t)(((rounded >> 13) - ((127u - 15u) << 10)) & 0x7fffu);
}
// one f16 plane of a device f32 weight tensor (n elements, the tensor's own [tap][Cout][Cin] layout), converted on the host
static bool f16_plane(ResNetModel &m, const float *dev, size_t n, void **out)
{
    std::vector<float> w(n);
    if (!hip_ok(hipMemcpy(w.data(), dev, n * 4, hipMemcpyDeviceToHost), "hipMemcpy(resnet weights, D2H)")) return false;
    std::vector<uint16_t> q(n);
    for (size_t i = 0; i < n; i++) q[i] = f16_rne_sat(w[i]);
    if (!hip_ok(hipMalloc(out, n * 2), "hipMalloc(resnet f16 weights)")) return false;
    m.owned.push_back(*out);
    return hip_ok(hipMemcpy(*out, q.data(), n * 2, hipMemcpyHostToDevice), "hipMemcpy(resnet f16 weights)");
}
static bool ensure_f16(ResNetModel &m)
{
    if (m.has_f16) return true;
    auto one = [&](ResConv &c) { return c.w16 || f16_plane(m, c.w, (size_t)c.ksize * c.ksize * c.cin * c.cout, &c.w16); };
    if (!m.stem_w16 && !f16_plane(m, m.stem_w, (size_t)64 * STEM_K, &m.stem_w16)) return false;
    for (ResBlock &k : m.blocks)
        if (!one(k.c1) || !one(k.c2) || !one(k.c3) || (k.has_sc && !one(k.sc))) return false;
    m.has_f16 = true;
    return true;
}

// One convolution of the forward, by activation type.  float: prec 0 (f32, bit-exact contract) or 3 (f16 operands: the model's f16
// planes, made by ensure_f16); uint16_t (f16act): IEEE binary16 activations in memory, always the f16 planes
static bool run_conv(const ResConv &c, int prec, const float *in, int N, int h, const float *resid, int relu, float *out, hipStream_t s)
{
    ConvArgs a{};
    a.in = in; a.N = N; a.h = h; a.w = h; a.Cin = c.cin; a.relu_in = 0; a.ksize = c.ksize; a.stride = c.stride; a.W = c.w; a.Cout = c.cout;
    a.scale = c.scale; a.shift = c.shift; a.resid = resid; a.rs = 0; a.relu_out = relu; a.out = out;
    if (prec == 3) { a.W = (const float *)c.w16; a.prec = 3; }
    return launch_conv(a, s);
}
static bool run_conv(const ResConv &c, int, const uint16_t *in, int N, int h, const uint16_t *resid, int relu, uint16_t *out, hipStream_t s)
{
    ConvF16Args a{};
    a.in = in; a.N = N; a.h = h; a.w = h; a.Cin = c.cin; a.ksize = c.ksize; a.stride = c.stride; a.W = (const uint16_t *)c.w16; a.Cout = c.cout;
    a.scale = c.scale; a.shift = c.shift; a.resid = resid; a.relu_out = relu; a.out = out;
    return launch_conv_f16act(a, s);
}
// ... and the stem's im2col: x (N, S, S, 3) -> col, STEM_K values per output pixel; the stem itself is then a 1x1 convolution
static void stem_im2col(const float *x, int N, int S, float *col, hipStream_t s)
{
    const size_t quads = (size_t)N * (S / 2) * (S / 2) * (STEM_K / 4);
    hipLaunchKernelGGL(resnet_im2col_kernel, dim3((unsigned)std::min<size_t>((quads + 255) / 256, 1u << 20)), dim3(256), 0, s, x, S, col, quads);
}
static void stem_im2col(const float *x, int N, int S, uint16_t *col, hipStream_t s)
{
    const size_t octs = (size_t)N * (S / 2) * (S / 2) * (STEM_K / 8);
    hipLaunchKernelGGL(resnet_im2col_f16_kernel, dim3((unsigned)std::min<size_t>((octs + 255) / 256, 1u << 20)), dim3(256), 0, s, x, S, (_Float16 *)col, octs);
}

// The forward on activations of type T: float, or uint16_t = IEEE binary16 bits in the first half of the buffers the f32 forms use (no
// allocation of its own, no host-side conversion).  Both run the same launches with the same buffer rotation.
template <typename T>
static int resnet_forward_as(const ResNetModel &m, int prec, const float *x, int N, int S, float *const bufs[4], float *col, float *prob, hipStream_t s)
{
    using KT = std::conditional_t<std::is_same<T, float>::value, float, _Float16>;      // the kernels' name for T
    T *a = (T *)bufs[0], *b = (T *)bufs[1], *t1 = (T *)bufs[2], *t2 = (T *)bufs[3];
    const int S2 = S / 2, S4 = S / 4;
    ResConv stem;
    stem.cin = STEM_K; stem.cout = 64; stem.w = m.stem_w; stem.w16 = m.stem_w16; stem.scale = m.stem_scale; stem.shift = m.stem_shift;
    stem_im2col(x, N, S, (T *)col, s);
    if (!run_conv(stem, prec, (const T *)col, N, S2, nullptr, 1, a, s)) return TMAT_E_ARG;
    const size_t ptotal = (size_t)N * S4 * S4 * 64;
    hipLaunchKernelGGL(resnet_pool_kernel<KT>, dim3((unsigned)std::min<size_t>((ptotal + 255) / 256, 16384)), dim3(256), 0, s, (const KT *)a, S2, 64, (KT *)b, ptotal);
    T *cur = b, *nxt = a;
    int h = S4;
    for (const ResBlock &k : m.blocks) {
        const int ho = h / k.c1.stride;
        const T *shortcut = cur;
        if (k.has_sc) {
            if (!run_conv(k.sc, prec, cur, N, h, nullptr, 0, t2, s)) return TMAT_E_ARG;
            shortcut = t2;
        }
        if (!run_conv(k.c1, prec, cur, N, h, nullptr, 1, t1, s)) return TMAT_E_ARG;
        if (!run_conv(k.c2, prec, t1, N, ho, nullptr, 1, nxt, s)) return TMAT_E_ARG;
        // c3 writes over t1 (its input is nxt), then the roles rotate: out -> cur
        if (!run_conv(k.c3, prec, nxt, N, ho, shortcut, 1, t1, s)) return TMAT_E_ARG;
        T *old = cur;
        cur = t1; t1 = old;
        h = ho;
    }
    hipLaunchKernelGGL(resnet_head_kernel<KT>, dim3(N), dim3(1024), 0, s, (const KT *)cur, h * h, m.feat, m.fc_w, m.fc_b, prob);
    return hipGetLastError() == hipSuccess ? TMAT_OK : TMAT_E_HIP;
}

// x (N, S, S, 3) f32 on the device -> prob (N) on the device; bufs: 4 activation buffers of N * (S/2)^2 * 64 floats; col: N * (S/2)^2 * 192
static int resnet_forward_dev(const ResNetModel &m, int mode, const float *x, int N, int S, float *const bufs[4], float *col, float *prob, hipStream_t s)
{
    const int prec = mode == TMAT_RESNET_PRECISION_F32 ? 0 : 3;
    if (m.feat > 1024) { set_error("resnet: head supports at most 1024 channels"); return TMAT_E_ARG; }
    if (prec == 3 && !m.has_f16) { set_error("resnet: the model has no f16 weights (tmat_resnet_set_precision makes them)"); return TMAT_E_ARG; }
    return mode == TMAT_RESNET_PRECISION_F16ACT ? resnet_forward_as<uint16_t>(m, prec, x, N, S, bufs, col, prob, s)
                                                : resnet_forward_as<float>(m, prec, x, N, S, bufs, col, prob, s);
}

int resnet_precision_from_env(Ctx *c)
{
    const char *e = getenv("TMAT_INV_DEPTH_PRECISION");
    if (!e || !strcmp(e, "f32")) return TMAT_OK;
    if (strcmp(e, "f16") && strcmp(e, "f16act")) { set_error("TMAT_INV_DEPTH_PRECISION must be f32, f16 or f16act"); return TMAT_E_ARG; }
    c->resnet_precision = strcmp(e, "f16") ? TMAT_RESNET_PRECISION_F16ACT : TMAT_RESNET_PRECISION_F16;      // no classifier is loaded yet: tmat_resnet_load makes the f16 planes
    return TMAT_OK;
}

int launch_resize_linear_dev(const uint16_t *din, int n, int H, int W, int oh, int ow, bool eight_bit, int *tab, uint16_t *dsm, hipStream_t s);      // cellarea_kernels.hip

}  // namespace tmat

using namespace tmat;

extern "C" {

int tmat_resnet_load(tmat_handle hd, const void *weights_blob, size_t n_bytes, int *model_id)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !weights_blob || !model_id) { set_error("tmat_resnet_load: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    std::map<std::string, Tensor> t;
    int patch = 0;
    if (!parse_blob(weights_blob, n_bytes, t, patch)) return TMAT_E_WEIGHTS;
    ResNetModel m;
    auto fail = [&]() { for (void *p : m.owned) hipFree(p); return TMAT_E_WEIGHTS; };
    // stem: BN folded with the convolution's bias
    auto sw = t.find("conv1.w"), sb = t.find("conv1.b"), sbn = t.find("conv1.bn");
    if (sw == t.end() || sb == t.end() || sbn == t.end() || sw->second.shape != std::vector<int>({7, 7, 3, 64}) || sbn->second.shape != std::vector<int>({4, 64}) ||
        sb->second.count != 64) { set_error("resnet weights: conv1 missing or malformed"); return fail(); }
    {
        std::vector<float> sc, sh;
        fold_bn_keras(sbn->second, sb->second, sc, sh);
        // (7, 7, 3, 64) = [147][64] as stored -> [64][192], k contiguous (conv_mfma_kernel's weight layout), zeros for k >= 147
        std::vector<float> wk((size_t)64 * STEM_K, 0.0f);
        for (int k = 0; k < STEM_TAPS; k++) for (int o = 0; o < 64; o++) wk[(size_t)o * STEM_K + k] = sw->second.data[(size_t)k * 64 + o];
        if (!up(m, wk, &m.stem_w) || !up(m, sc, &m.stem_scale) || !up(m, sh, &m.stem_shift)) return fail();
    }
    int cin = 64;
    for (int stage = 2;; stage++) {
        if (!t.count("s" + std::to_string(stage) + "b1.c1.w")) break;
        for (int blk = 1;; blk++) {
            const std::string p = "s" + std::to_string(stage) + "b" + std::to_string(blk);
            if (!t.count(p + ".c1.w")) break;
            ResBlock k;
            const int stride = (blk == 1 && stage > 2) ? 2 : 1;
            k.has_sc = blk == 1;
            if (!load_conv(m, t, p + ".c1", 1, stride, cin, k.c1) || !load_conv(m, t, p + ".c2", 3, 1, k.c1.cout, k.c2) || !load_conv(m, t, p + ".c3", 1, 1, k.c2.cout, k.c3)) return fail();
            if (k.has_sc) { if (!load_conv(m, t, p + ".c0", 1, stride, cin, k.sc) || k.sc.cout != k.c3.cout) { set_error("resnet weights: bad shortcut " + p); return fail(); } }
            else if (k.c3.cout != cin) { set_error("resnet weights: identity block changes the channel count: " + p); return fail(); }
            cin = k.c3.cout;
            m.blocks.push_back(k);
        }
    }
    auto fw = t.find("fc.w"), fb = t.find("fc.b");
    if (m.blocks.empty() || fw == t.end() || fb == t.end() || (int)fw->second.count != cin || fb->second.count != 1) { set_error("resnet weights: head missing or malformed"); return fail(); }
    m.feat = cin;
    m.fc_b = fb->second.data[0];
    if (!up(m, std::vector<float>(fw->second.data, fw->second.data + cin), &m.fc_w)) return fail();
    if (c->resnet_precision != TMAT_RESNET_PRECISION_F32 && !ensure_f16(m)) return fail();
    c->resnets.push_back(std::move(m));
    *model_id = (int)c->resnets.size() - 1;
    return TMAT_OK;
}

int tmat_resnet_set_precision(tmat_handle hd, int mode)
{
    Ctx *c = (Ctx *)hd;
    if (!c || (mode != TMAT_RESNET_PRECISION_F32 && mode != TMAT_RESNET_PRECISION_F16 && mode != TMAT_RESNET_PRECISION_F16ACT)) {
        set_error("tmat_resnet_set_precision: needs a handle and mode TMAT_RESNET_PRECISION_F32, TMAT_RESNET_PRECISION_F16 or TMAT_RESNET_PRECISION_F16ACT");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    { const int rc = tmat_sync(hd); if (rc) return rc; }      // nothing in flight runs across the switch
    if (mode != TMAT_RESNET_PRECISION_F32)          // both 16-bit modes multiply the same f16 weight planes
        for (ResNetModel &m : c->resnets) if (!ensure_f16(m)) return TMAT_E_HIP;
    c->resnet_precision = mode;
    return TMAT_OK;
}

// Stage-wise test entry point: ONE launch_conv on host buffers.  x (n, hh, ww, cin); w in the Keras layout (ksize, ksize, cin, cout);
// scale nullable (plain bias); resid nullable, (n, hh / stride, ww / stride, cout); out the same shape.  prec 0: f32, 3: f16 operands,
// 4: the f16act convolution -- x (after the load-side ReLU, which commutes with the rounding) and resid rounded to f16 on the host, f16
// device buffers, the f16 output widened to f32 on the host.
int tmat_conv2d(tmat_handle hd, int prec, const float *x, int n, int hh, int ww, int cin, const float *w, int ksize, int stride, int cout,
                const float *scale, const float *shift, const float *resid, int relu_in, int relu_out, float *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !x || !w || !shift || !out || (prec != 0 && prec != 3 && prec != 4) || n < 1 || hh < 1 || ww < 1 || cin < 1 || cout < 1 || (ksize != 1 && ksize != 3) ||
        (stride != 1 && stride != 2) || hh % stride || ww % stride) {
        set_error("tmat_conv2d: bad argument (prec 0, 3 or 4, ksize 1 or 3, stride 1 or 2)");
        return TMAT_E_ARG;
    }
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nx = (size_t)n * hh * ww * cin, nw = (size_t)ksize * ksize * cin * cout, no = (size_t)n * (hh / stride) * (ww / stride) * cout;
    const bool f16act = prec == 4;
    const size_t asz = f16act ? 2 : 4, wsz = prec >= 3 ? 2 : 4;       // bytes per activation and per weight on the device
    DevScope mem(c->ws_pool, s);
    auto f16 = [&mem](const float *v, size_t count, bool relu) {
        uint16_t *q = mem.host<uint16_t>(count);
        for (size_t i = 0; i < count; i++) q[i] = f16_rne_sat(relu && !(v[i] > 0.f) ? 0.f : v[i]);
        return (const char *)q;
    };
    // how each mode rounds its operands on the host: prec 3 the weights; prec 4 also x (after the load-side ReLU) and resid
    std::vector<float> wk = k_contiguous(w, ksize * ksize, cin, cout);
    const char *hw = prec >= 3 ? f16(wk.data(), nw, false) : (const char *)mem.keep(std::move(wk));
    const char *hx = f16act ? f16(x, nx, relu_in != 0) : (const char *)x;
    const char *hr = resid && f16act ? f16(resid, no, false) : (const char *)resid;
    uint16_t *oq = f16act ? mem.host<uint16_t>(no) : nullptr;
    char *dx = mem.alloc_from(hx, nx * asz), *dw = mem.alloc_from(hw, nw * wsz);
    float *dsh = mem.alloc_from(shift, cout), *dsc = scale ? mem.alloc_from(scale, cout) : nullptr;
    char *dr = hr ? mem.alloc_from(hr, no * asz) : nullptr, *dout = mem.alloc<char>(no * asz);
    if (!mem.ok) return TMAT_E_HIP;
    bool launched;
    if (f16act) {
        ConvF16Args a{};
        a.in = (uint16_t *)dx; a.N = n; a.h = hh; a.w = ww; a.Cin = cin; a.ksize = ksize; a.stride = stride; a.W = (uint16_t *)dw; a.Cout = cout;
        a.scale = dsc; a.shift = dsh; a.resid = (uint16_t *)dr; a.relu_out = relu_out != 0; a.out = (uint16_t *)dout;
        launched = launch_conv_f16act(a, s);
    } else {
        ConvArgs a{};
        a.in = (float *)dx; a.N = n; a.h = hh; a.w = ww; a.Cin = cin; a.relu_in = relu_in != 0; a.ksize = ksize; a.stride = stride; a.W = (const float *)dw;
        a.Cout = cout; a.scale = dsc; a.shift = dsh; a.resid = (float *)dr; a.rs = 0; a.relu_out = relu_out != 0; a.out = (float *)dout; a.prec = prec;
        launched = launch_conv(a, s);
    }
    if (!launched) return TMAT_E_ARG;
    mem.check(hipGetLastError(), "tmat_conv2d launch");
    mem.d2h(f16act ? (void *)oq : (void *)out, dout, no * asz);
    if (mem.finish()) return TMAT_E_HIP;
    for (size_t i = 0; oq && i < no; i++) out[i] = (float)__builtin_bit_cast(_Float16, oq[i]);
    return TMAT_OK;
}

int tmat_resnet_predict(tmat_handle hd, int model_id, const float *x, int n, int size, float *prob)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !x || !prob || n < 0 || size < 32 || size % 32 || model_id < 0 || model_id >= (int)c->resnets.size()) { set_error("tmat_resnet_predict: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nx = (size_t)n * size * size * 3, nb = (size_t)n * (size / 2) * (size / 2) * 64;
    DevScope mem(c->ws_pool, s);
    float *dx = mem.alloc_from(x, nx), *dp = mem.alloc<float>(n), *col = mem.alloc<float>(nb * 3), *bufs[4];      // col: 192 = 3 x 64 values per stem output pixel
    for (float *&b : bufs) b = mem.alloc<float>(nb);
    if (!mem.ok) return TMAT_E_HIP;
    int rc = resnet_forward_dev(c->resnets[model_id], c->resnet_precision, dx, n, size, bufs, col, dp, s);
    if (rc) return rc;
    mem.d2h(prob, dp, n * 4);
    return mem.finish();
}

}  // extern "C"

// stacks[k] (Zs[k], H, W) u16 host, k < n_stacks: uploaded back to back (Z = their sum) -- every step of the tool is per slice
static int inv_depth_impl(tmat_handle hd, const int *model_ids, int n_models, const uint16_t *const *stacks, const int *Zs, int n_stacks, int Z, int H, int W,
                          int size, float *probs, float *x_out)
{
    Ctx *c = (Ctx *)hd;
    for (int i = 0; i < n_models; i++) if (model_ids[i] < 0 || model_ids[i] >= (int)c->resnets.size()) { set_error("tmat_inv_depth_predict: unknown model id"); return TMAT_E_ARG; }
    if (Z == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int CH = 128;                                    // slices per forward: M = 128 x 16^2 rows at the deepest stage (round 2: 32, launch bound)
    const size_t npx = (size_t)size * size;
    // cv2.resize(img, img_hw, cv2.INTER_LANCZOS4) (data_prep.py:36): the third positional parameter is `dst`: bilinear
    const int nb = std::min(Z, CH);
    // workspaces live on the handle between calls (tmat_ctx.h:ws_get); the scope carries the copies, and a failed call leaves nothing in
    // flight on them
    uint16_t *din = (uint16_t *)ws_get(c, WS_INV_IN, (size_t)Z * H * W * 2), *dsm = (uint16_t *)ws_get(c, WS_INV_SMALL, (size_t)Z * npx * 2);
    int *itab = (int *)ws_get(c, WS_INV_TAB, (size_t)size * 2 * 4 * 4), *mnmx = (int *)ws_get(c, WS_INV_MNMX, (size_t)Z * 2 * 4);
    float *dx = (float *)ws_get(c, WS_INV_X, (size_t)Z * npx * 3 * 4), *dp = (float *)ws_get(c, WS_INV_PROB, (size_t)Z * n_models * 4), *bufs[4];
    for (int i = 0; i < 4; i++) bufs[i] = (float *)ws_get(c, (ToolWs)(WS_INV_BUF0 + i), (size_t)nb * (size / 2) * (size / 2) * 64 * 4);
    float *col = (float *)ws_get(c, WS_INV_COL, (size_t)nb * (size / 2) * (size / 2) * STEM_K * 4);
    if (!din || !dsm || !itab || !mnmx || !dx || !dp || !bufs[0] || !bufs[1] || !bufs[2] || !bufs[3] || !col) return TMAT_E_HIP;
    DevScope mem(c->ws_pool, s);
    size_t z0 = 0;
    for (int k = 0; k < n_stacks; k++) {
        mem.h2d(din + z0 * H * W, stacks[k], (size_t)Zs[k] * H * W * 2);
        z0 += (size_t)Zs[k];
    }
    // cv::resize takes INTER_AREA's integer mean for an exact halving on both axes (a 512 x 512 slice at the configured 256 x 256);
    // 8-bit sources (tmat_set_input_depth(h, 8)) take its fixed-point bilinear arithmetic
    if (!mem.ok || launch_resize_linear_dev(din, Z, H, W, size, size, c->input_sat == 255.f, itab, dsm, s)) { set_error("tmat_inv_depth_predict: upload failed"); return TMAT_E_HIP; }
    const int blocks = (int)((npx + 255) / 256);
    hipLaunchKernelGGL(minmax_u16_img_kernel, dim3(Z), dim3(256), 0, s, dsm, (int)npx, mnmx, mnmx + Z);
    hipLaunchKernelGGL(inv_prep_kernel, dim3(blocks < 1024 ? blocks : 1024, Z), dim3(256), 0, s, dsm, (int)npx, mnmx, mnmx + Z, dx);
    for (int mi = 0; mi < n_models; mi++)
        for (int z = 0; z < Z; z += CH) {
            const int rc = resnet_forward_dev(c->resnets[model_ids[mi]], c->resnet_precision, dx + (size_t)z * npx * 3, std::min(CH, Z - z), size, bufs, col, dp + (size_t)mi * Z + z, s);
            if (rc) return rc;
        }
    float *ph = mem.host<float>((size_t)Z * n_models);
    mem.d2h(ph, dp, (size_t)Z * n_models * 4);
    mem.d2h(x_out, dx, (size_t)Z * npx * 3 * 4);
    if (mem.finish()) return TMAT_E_HIP;
    for (int z = 0; z < Z; z++) for (int mi = 0; mi < n_models; mi++) probs[(size_t)z * n_models + mi] = ph[(size_t)mi * Z + z];     // (Z, n_models)
    return TMAT_OK;
}

extern "C" {

int tmat_inv_depth_predict(tmat_handle hd, const int *model_ids, int n_models, const uint16_t *stack, int Z, int H, int W, int size, float *probs, float *x_out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !model_ids || !stack || !probs || n_models < 1 || Z < 0 || H < 1 || W < 1 || size < 32 || size % 32) { set_error("tmat_inv_depth_predict: bad argument"); return TMAT_E_ARG; }
    return inv_depth_impl(hd, model_ids, n_models, &stack, &Z, 1, Z, H, W, size, probs, x_out);
}

int tmat_inv_depth_predict_multi(tmat_handle hd, const int *model_ids, int n_models, const uint16_t *const *stacks, const int *Zs, int n_stacks, int H, int W,
                                 int size, float *probs)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !model_ids || !stacks || !Zs || !probs || n_models < 1 || n_stacks < 0 || H < 1 || W < 1 || size < 32 || size % 32) {
        set_error("tmat_inv_depth_predict_multi: bad argument"); return TMAT_E_ARG;
    }
    long long Z = 0;
    for (int k = 0; k < n_stacks; k++) {
        if (Zs[k] < 0 || (Zs[k] > 0 && !stacks[k])) { set_error("tmat_inv_depth_predict_multi: bad stack"); return TMAT_E_ARG; }
        Z += Zs[k];
    }
    if (Z > 0x7fffffffLL / ((long long)size * size)) { set_error("tmat_inv_depth_predict_multi: too many slices"); return TMAT_E_ARG; }
    return inv_depth_impl(hd, model_ids, n_models, stacks, Zs, n_stacks, (int)Z, H, W, size, probs, nullptr);
}

}  // extern "C"
