// The convolution of the NARROW UNet layers (gfx950): channel counts that are multiples of 16 -- what launch_conv (unet_kernels.hip) refuses.
//
// build_UNetXception's own default is filter_counts (32, 64, 128, 256), and the training notebook searches (16, 32, 64, 128) too: their
// first down blocks and last up blocks have 16 and 32 channels, where conv_mfma_kernel wants Cout % 64 == 0 and a K step of two 32-channel
// chunks.  A kernel of its own file, not further instantiations of conv_mfma_kernel: DESIGN 11 records that a path merely compiled into
// that kernel slowed launches that never ran it.  The UNet driver (tmat_api.cpp:conv) launches this one only where conv_mfma_takes says no.
//
// Arithmetic: the f32 contract of unet_kernels.hip, bit for bit oracle/unet.py:_conv / _conv_subpixel -- one k-ordered chain of
// single-rounding fmaf per output on v_mfma_f32_32x32x2_f32: input channels in blocks of 32 (a last block of 16 is simply short), inside
// a block tap-major, inside (block, tap) every group of 8 channels in the order 0, 4, 1, 5, 2, 6, 3, 7; out-of-image taps multiply zeros.
// Epilogue: scale ? fmaf(acc, scale, shift) : acc + shift, + resid, ReLU.
//
// Layout: a wave owns 32 consecutive pixels of its segment and, per pass over K, NCT column tiles of 32 output channels (a Cout that is
// no multiple of 32 ends in a tile whose upper 16 rows multiply zero weights and are not stored).  The WEIGHTS are the A operand (row =
// output channel = lane & 31, k = lane >> 5), the PIXELS the B operand (column = lane & 31): lane l reads the four channels
// 8 g + 4 (l >> 5) .. + 3 of its pixel and of its weight row with one 16-byte load each and feeds them to four MFMAs, which therefore
// consume the channel pairs (8 g + e, 8 g + 4 + e), e = 0 .. 3 -- the order above.  A lane ends up with ITS pixel's output channels
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) in accumulator register r: four runs of four consecutive channels, so the epilogue needs no transposition
// through LDS and stores 16 bytes at a time.  No LDS at all: the operands of these layers are short (K = 16 .. 576) and the weights stay
// in the L1 / L2.  The pointwise launches run at 0.6 - 0.9 of their HBM bound that way; the 3x3 and sub-pixel ones pay for the fragment
// loads' line lookups and reach 0.2 - 0.4 of theirs (DESIGN 4.1.8 has the table and what would come next).
// Pixel <-> (patch, row, column) is per lane, by exact multiply-shift division: any width, any first column, any M.
#include "dev_guard.h"
#include "tmat_internal.h"
#include "../../include/tmat.h"

#include <type_traits>

namespace tmat {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NW_WAVES = 4;             // waves per workgroup
constexpr int NW_BM = 32 * NW_WAVES;    // pixels per workgroup: the pixel tile

// exact n / d for 0 <= n < 2^31 and a launch constant d >= 2 (unet_kernels.hip:FastDiv has the proof)
struct NDiv { unsigned mul; int sh; };
NDiv make_ndiv(int d)
{
    int l = 0;
    while ((1ll << l) < d) l++;
    const unsigned long long num = 1ull << (31 + l);
    return NDiv{(unsigned)((num + (unsigned long long)d - 1) / (unsigned long long)d), l - 1};
}
__device__ __forceinline__ int ndiv(int n, NDiv f) { return (int)(__umulhi((unsigned)n, f.mul) >> f.sh); }

// x > 0 ? x : +0.0 (negative values and -0.0 are negative as signed integers; no NaNs on this path)
__device__ __forceinline__ float relu0(float v) { return __builtin_bit_cast(float, max(__builtin_bit_cast(int, v), 0)); }
__device__ __forceinline__ float4 relu0(float4 v) { return make_float4(relu0(v.x), relu0(v.y), relu0(v.z), relu0(v.w)); }

// KS 1 / 3: ksize; KS 2: the sub-pixel form (blockIdx.y = output parity class, M enumerates stored pixels).  ROI: the region form, with the
// meaning conv_mfma_kernel<..., ROI> gives the table -- tile mt belongs to the last segment whose mt0 <= mt.
// grid: (pixel tiles, KS == 2 ? 4 : 1); a workgroup walks the groups of 32 NCT output channels of its pixels one after the other
template <int KS, bool RELU, bool ROI, int NCT>
__global__ __launch_bounds__(64 * NW_WAVES) void conv_narrow_kernel(ConvArgs a, int Mf, int Ho, int Wo, NDiv dHWf, NDiv dWf,
                                                                     std::conditional_t<ROI, RoiSegs, RoiNone> roi)
{
    constexpr int TAPS = KS * KS;
    const int mt = blockIdx.x;
    int M = Mf, HW = Ho * Wo, Wr = Wo, sn = 0, sy0 = 0, sx0 = 0, mtl = mt;
    NDiv dHW = dHWf, dW = dWf;
    if constexpr (ROI) {
        int si = 0;
        for (int k = 1; k < roi.nseg; k++) si = mt >= roi.s[k].mt0 ? k : si;        // scalar: mt and the table are uniform
        M = roi.s[si].M; Wr = roi.s[si].rw; HW = roi.s[si].rh * Wr;
        sn = roi.s[si].p0; sy0 = roi.s[si].y0; sx0 = roi.s[si].x0; mtl = mt - roi.s[si].mt0;
        dHW = NDiv{roi.s[si].dhw_mul, roi.s[si].dhw_sh}; dW = NDiv{roi.s[si].dw_mul, roi.s[si].dw_sh};
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mw = mtl * NW_BM + wave * 32;             // first pixel of the wave
    if (mw >= M) return;                                // (wave-uniform; the kernel has no barrier)
    const int px = lane & 31, hi = lane >> 5;
    const bool ok = mw + px < M;
    // pixel -> (patch, row, column) of the layer's output (sub-pixel form: of the stored tensor); lanes past M take the wave's first pixel
    // and neither load nor store
    int n, y, x;
    {
        const int m = ok ? mw + px : mw;
        n = ndiv(m, dHW);
        const int r = m - n * HW;
        y = ndiv(r, dW);
        x = r - y * Wr + sx0;
        n += sn; y += sy0;
    }
    const int spy = KS == 2 ? (int)(blockIdx.y >> 1) : 0, spx = KS == 2 ? (int)(blockIdx.y & 1) : 0;
    // the stored pixel tap 0 reads, and per tap whether it lies inside the image
    const int iy = KS == 3 ? y - 1 : KS == 2 ? y + spy - 1 : y * a.stride;
    const int ix = KS == 3 ? x - 1 : KS == 2 ? x + spx - 1 : x * a.stride;
    const float *const ap0 = a.in + (((long long)n * a.h + iy) * a.w + ix) * a.Cin + 4 * hi;
    unsigned inside = 0;
#pragma unroll
    for (int tp = 0; tp < TAPS; tp++) {
        const int ty = iy + tp / KS, tx = ix + tp % KS;
        if (ok && ty >= 0 && ty < a.h && tx >= 0 && tx < a.w) inside |= 1u << tp;
    }
    const float *const wt = a.W + (KS == 2 ? (size_t)blockIdx.y * 4 * a.Cout * a.Cin : (size_t)0) + 4 * hi;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int c0 = 0; c0 < a.Cout; c0 += 32 * NCT) {
        f32x16 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[ct][r] = 0.f;
        // this lane's weight row of every column tile (rows past Cout: zeros)
        const float *wrow[NCT];
        bool wok[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
            const int co = c0 + ct * 32 + px;
            wok[ct] = co < a.Cout;
            wrow[ct] = wt + (size_t)(wok[ct] ? co : 0) * a.Cin;
        }
        for (int cb = 0; cb < a.Cin; cb += 32) {
            const int ng = min(4, (a.Cin - cb) >> 3);       // groups of 8 channels in this block: 4, or 2 in a short last block
#pragma unroll
            for (int tp = 0; tp < TAPS; tp++) {
                const bool in = (inside >> tp) & 1u;
                const float *const ap = ap0 + ((long long)(tp / KS) * a.w + tp % KS) * a.Cin + cb;
                const size_t wo = (size_t)tp * a.Cout * a.Cin + cb;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    if (g >= ng) break;                     // (uniform)
                    float4 xv = zero4;
                    if (in) xv = *reinterpret_cast<const float4 *>(ap + 8 * g);
                    if (RELU) xv = relu0(xv);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++) {
                        float4 wv = zero4;
                        if (wok[ct]) wv = *reinterpret_cast<const float4 *>(wrow[ct] + wo + 8 * g);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, xv.x, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, xv.y, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.z, xv.z, acc[ct], 0, 0, 0);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.w, xv.w, acc[ct], 0, 0, 0);
                    }
                }
            }
        }
        // epilogue: register r of tile ct is channel c0 + 32 ct + (r & 3) + 8 (r >> 2) + 4 hi of this lane's pixel
        if (ok) {
            const int rH = Ho >> a.rs, rW = Wo >> a.rs;
            const size_t opix = KS == 2 ? ((size_t)n * 2 * Ho + 2 * y + spy) * (2 * (size_t)Wo) + 2 * x + spx : ((size_t)n * Ho + y) * Wo + x;
            const size_t rpix = ((size_t)n * rH + (y >> a.rs)) * rW + (x >> a.rs);
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int co = c0 + ct * 32 + 8 * q + 4 * hi;
                    if (co >= a.Cout) continue;             // (Cout % 16 == 0: four channels are inside or outside together)
                    float4 v = make_float4(acc[ct][4 * q], acc[ct][4 * q + 1], acc[ct][4 * q + 2], acc[ct][4 * q + 3]);
                    const float4 sh = *reinterpret_cast<const float4 *>(a.shift + co);
                    if (a.scale) {
                        const float4 sc = *reinterpret_cast<const float4 *>(a.scale + co);
                        v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
                    } else {
                        v.x = v.x + sh.x; v.y = v.y + sh.y; v.z = v.z + sh.z; v.w = v.w + sh.w;
                    }
                    if (a.resid) {
                        const float4 rv = *reinterpret_cast<const float4 *>(a.resid + rpix * a.Cout + co);
                        v.x = v.x + rv.x; v.y = v.y + rv.y; v.z = v.z + rv.z; v.w = v.w + rv.w;
                    }
                    if (a.relu_out) v = relu0(v);
                    *reinterpret_cast<float4 *>(a.out + opix * a.Cout + co) = v;
                    if (KS != 2 && a.out_relu) *reinterpret_cast<float4 *>(a.out_relu + opix * a.Cout + co) = relu0(v);
                }
        }
    }
}

template <int KS, bool ROI, int NCT>
void launch_narrow_inst(const ConvArgs &a, int M, int Ho, int Wo, dim3 grid, std::conditional_t<ROI, RoiSegs, RoiNone> roi, hipStream_t s)
{
    const NDiv dHW = make_ndiv(Ho * Wo), dW = make_ndiv(Wo);
    if (a.relu_in) hipLaunchKernelGGL((conv_narrow_kernel<KS, true, ROI, NCT>), grid, dim3(64 * NW_WAVES), 0, s, a, M, Ho, Wo, dHW, dW, roi);
    else hipLaunchKernelGGL((conv_narrow_kernel<KS, false, ROI, NCT>), grid, dim3(64 * NW_WAVES), 0, s, a, M, Ho, Wo, dHW, dW, roi);
}

template <int KS>
void launch_narrow_ks(const ConvArgs &a, int M, int Ho, int Wo, hipStream_t s, const RoiSegs *roi)
{
    int nMt = (M + NW_BM - 1) / NW_BM;
    RoiSegs rs{};
    if (roi) {          // the pixel tiles of the segments one after the other, a tile never straddling two of them
        rs = *roi;
        nMt = 0;
        for (int i = 0; i < rs.nseg; i++) {
            RoiSeg &g = rs.s[i];
            g.M = g.np * g.rh * g.rw;
            g.mt0 = nMt;
            nMt += (g.M + NW_BM - 1) / NW_BM;
            const NDiv f = make_ndiv(g.rh * g.rw), fw = make_ndiv(g.rw);
            g.dhw_mul = f.mul; g.dhw_sh = f.sh; g.dw_mul = fw.mul; g.dw_sh = fw.sh;
        }
    }
    // up to 32 output channels: one column tile per pass over K; above: two, so that a pixel fragment feeds eight MFMAs
    const bool two = a.Cout > 32;
    // every column group of a pixel tile in ONE workgroup (the loop over c0): the tile's pixels are fetched by one CU
    const dim3 grid(nMt, KS == 2 ? 4 : 1, 1);
    if (roi) {
        if (two) launch_narrow_inst<KS, true, 2>(a, M, Ho, Wo, grid, rs, s);
        else launch_narrow_inst<KS, true, 1>(a, M, Ho, Wo, grid, rs, s);
    } else {
        if (two) launch_narrow_inst<KS, false, 2>(a, M, Ho, Wo, grid, RoiNone{}, s);
        else launch_narrow_inst<KS, false, 1>(a, M, Ho, Wo, grid, RoiNone{}, s);
    }
}

}  // namespace

bool conv_narrow_takes(const ConvArgs &a)
{
    if (a.stride < 1 || a.stride > 2) return false;
    const int Ho = a.h / a.stride, Wo = a.w / a.stride;
    const long long Mll = (long long)a.N * Ho * Wo;
    const bool form = (a.ksize == 3 && a.stride == 1) || (a.ksize == 2 && a.stride == 1 && !a.resid && !a.out_relu) ||
                      (a.ksize == 1 && (a.stride == 1 || (!((a.h | a.w) & 1))));
    return form && a.prec == 0 && a.Cin >= 16 && a.Cin % 16 == 0 && a.Cout >= 16 && a.Cout % 16 == 0 && a.N >= 1 && a.h >= 1 && a.w >= 1 &&
           Mll > 0 && Mll <= 0x7fffffffLL / 2 && (a.rs == 0 || a.rs == 1) && !(a.resid && a.rs && ((Ho | Wo) & 1)) && Wo >= 2;
}

bool launch_conv_narrow(const ConvArgs &a, hipStream_t s, const RoiSegs *roi)
{
    if (!conv_narrow_takes(a)) {
        set_error("launch_conv_narrow: unsupported shape");
        return false;
    }
    const int Ho = a.h / a.stride, Wo = a.w / a.stride;
    const int M = a.N * Ho * Wo;
    if (roi) {      // launch_conv's rule: every segment inside the batch and the patch, at least two pixels wide; patch ranges in ascending
                    // order, or the previous segment's range again with a rectangle disjoint from every other one of that range
        bool ok = roi->nseg >= 1 && roi->nseg <= ROI_MAX_SEGS;
        for (int i = 0, p = 0, first = 0; ok && i < roi->nseg; i++) {
            const RoiSeg &g = roi->s[i];
            ok = g.np >= 1 && g.p0 >= 0 && g.p0 + g.np <= a.N && g.y0 >= 0 && g.x0 >= 0 && g.rh >= 1 && g.rw >= 2 && g.y0 + g.rh <= Ho && g.x0 + g.rw <= Wo;
            if (ok && i > 0 && g.p0 == roi->s[first].p0 && g.np == roi->s[first].np) {
                for (int j = first; ok && j < i; j++) {
                    const RoiSeg &o = roi->s[j];
                    ok = g.y0 >= o.y0 + o.rh || o.y0 >= g.y0 + g.rh || g.x0 >= o.x0 + o.rw || o.x0 >= g.x0 + g.rw;
                }
            } else {
                ok = ok && g.p0 >= p;
                first = i;
            }
            p = g.p0 + g.np;
        }
        if (!ok) { set_error("launch_conv_narrow: bad region table"); return false; }
    }
    if (a.ksize == 3) launch_narrow_ks<3>(a, M, Ho, Wo, s, roi);
    else if (a.ksize == 2) launch_narrow_ks<2>(a, M, Ho, Wo, s, roi);
    else launch_narrow_ks<1>(a, M, Ho, Wo, s, roi);
    return true;
}

}  // namespace tmat
