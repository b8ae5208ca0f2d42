// Tree overlay on the device: one workgroup per 64 x 16 canvas tile composites the image's segments over the min-max rescaled
// background (DESIGN.md "Tree overlay and barcode pictures").  The segments of the image are scanned tile-centrically in chunks of one
// per thread; the ones whose bounding box touches the tile are compacted into LDS IN SEGMENT ORDER (wave ballots + a prefix over the
// waves), so painter's order never depends on scheduling and no atomics or global lists are involved.  Each thread owns four
// neighbouring pixels of a row and writes their twelve bytes as three dwords: a wave writes 4 rows x 192 contiguous bytes.
// barcode_kernel (further down) fills the barcode canvases from the host's rectangle tables.
#include "overlay.h"

#include <algorithm>

namespace tmat {
namespace {

constexpr int OVL_THREADS = 256;

__device__ inline float bg_value(const void *bg, int dtype, size_t i)
{
    return dtype == 0 ? (float)((const uint16_t *)bg)[i] : ((const float *)bg)[i];
}

// order-preserving map float -> uint32 (for atomicMin / atomicMax, whose result does not depend on the order of the updates)
__device__ inline uint32_t f2ord(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ inline float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__global__ void ovl_minmax_init(uint32_t *ord, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { ord[2 * i] = 0xffffffffu; ord[2 * i + 1] = 0u; }
}

__global__ __launch_bounds__(OVL_THREADS) void ovl_minmax(const void *bg, int dtype, size_t per, uint32_t *ord)
{
    const int img = blockIdx.y;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (size_t i = (size_t)blockIdx.x * OVL_THREADS + threadIdx.x; i < per; i += (size_t)gridDim.x * OVL_THREADS) {
        uint32_t k = f2ord(bg_value(bg, dtype, (size_t)img * per + i));
        lo = min(lo, k); hi = max(hi, k);
    }
    __shared__ uint32_t slo[OVL_THREADS], shi[OVL_THREADS];
    slo[threadIdx.x] = lo; shi[threadIdx.x] = hi;
    __syncthreads();
    for (int st = OVL_THREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            slo[threadIdx.x] = min(slo[threadIdx.x], slo[threadIdx.x + st]);
            shi[threadIdx.x] = max(shi[threadIdx.x], shi[threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { atomicMin(&ord[2 * img], slo[0]); atomicMax(&ord[2 * img + 1], shi[0]); }
}

__global__ void ovl_minmax_finish(const uint32_t *ord, float *mnmx, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * n) mnmx[i] = ord2f(ord[i]);
}

struct alignas(4) Bytes12 { uint32_t a, b, c; };

__global__ __launch_bounds__(OVL_THREADS) void ovl_render(const void *bg, int dtype, const float *mnmx, int bh, int bw, const OverlaySeg *segs,
                                                          const int *seg_offsets, int vh, int vw, float rp, uint8_t *rgb)
{
    __shared__ OverlaySeg lseg[OVL_THREADS];
    __shared__ int wave_cnt[OVL_THREADS / 64];
    const int img = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * OVL_TW, y0 = blockIdx.y * OVL_TH;
    const int px0 = x0 + (tid & 15) * 4, py = y0 + (tid >> 4);
    const bool row_in = py < vh;

    // background: nearest sample of the rescaled image
    float C[4][3];
    {
        const float mn = mnmx[2 * img], mx = mnmx[2 * img + 1];
        const int sy = ovl_sample_index(row_in ? py : vh - 1, bh, vh);
        for (int j = 0; j < 4; j++) {
            const int px = px0 + j < vw ? px0 + j : vw - 1;
            const int sx = ovl_sample_index(px, bw, vw);
            const float g = ovl_grey(bg_value(bg, dtype, ((size_t)img * bh + sy) * bw + sx), mn, mx);
            C[j][0] = g; C[j][1] = g; C[j][2] = g;
        }
    }
    // tile rectangle grown by the capsule's reach and one pixel of slack: a segment outside it covers no pixel centre of the tile
    const float reach = rp + 1.0f;
    const float tx0 = (float)x0 - reach, tx1 = (float)(x0 + OVL_TW - 1) + reach;
    const float ty0 = (float)y0 - reach, ty1 = (float)(y0 + OVL_TH - 1) + reach;
    const int s0 = seg_offsets[img], s1 = seg_offsets[img + 1];
    const float cy = (float)py;
    for (int base = s0; base < s1; base += OVL_THREADS) {
        OverlaySeg mine;
        bool hit = false;
        if (base + tid < s1) {
            mine = segs[base + tid];
            hit = fminf(mine.x1, mine.x2) <= tx1 && fmaxf(mine.x1, mine.x2) >= tx0 && fminf(mine.y1, mine.y2) <= ty1 && fmaxf(mine.y1, mine.y2) >= ty0;
        }
        const unsigned long long ball = __ballot(hit);
        if (lane == 0) wave_cnt[wave] = __popcll(ball);
        __syncthreads();
        int before = 0, total = 0;
        for (int wv = 0; wv < OVL_THREADS / 64; wv++) { if (wv < wave) before += wave_cnt[wv]; total += wave_cnt[wv]; }
        if (hit) lseg[before + __popcll(ball & ((1ull << lane) - 1ull))] = mine;
        __syncthreads();
        for (int k = 0; k < total; k++) {
            const OverlaySeg sg = lseg[k];
            for (int j = 0; j < 4; j++) {
                const float a = ovl_coverage(sg, (float)(px0 + j), cy, rp);
                C[j][0] = ovl_blend(C[j][0], sg.r, a);
                C[j][1] = ovl_blend(C[j][1], sg.g, a);
                C[j][2] = ovl_blend(C[j][2], sg.b, a);
            }
        }
        __syncthreads();        // lseg / wave_cnt are rewritten by the next chunk
    }
    if (!row_in || px0 >= vw) return;
    uint8_t o[12];
    for (int j = 0; j < 4; j++)
        for (int ch = 0; ch < 3; ch++) o[3 * j + ch] = (uint8_t)floorf(C[j][ch] + 0.5f);
    uint8_t *dst = rgb + (((size_t)img * vh + py) * vw + px0) * 3;
    if ((vw & 3) == 0) {        // px0 is a multiple of 4: the twelve bytes are dword-aligned and all four pixels are on the canvas
        Bytes12 v;
        v.a = o[0] | (o[1] << 8) | (o[2] << 16) | ((uint32_t)o[3] << 24);
        v.b = o[4] | (o[5] << 8) | (o[6] << 16) | ((uint32_t)o[7] << 24);
        v.c = o[8] | (o[9] << 8) | (o[10] << 16) | ((uint32_t)o[11] << 24);
        *(Bytes12 *)dst = v;
    } else {
        const int npx = vw - px0 < 4 ? vw - px0 : 4;
        for (int k = 0; k < 3 * npx; k++) dst[k] = o[k];
    }
}

// Barcode canvases: HBM-bound fill, no LDS.  A thread owns 16 consecutive bytes of the FLAT batch buffer (pictures, rows and pixels run
// through: S * 3 is rarely a multiple of 16) and writes them with one 16-byte store; the last, short group of the buffer is written
// byte by byte.  The bar of a canvas row comes from index arithmetic -- row y (from the bottom) can only belong to bar floor((y + 0.5) /
// pitch) -- plus a check of its two neighbours against the table's own row ranges, which absorbs the rounding of the division.
__device__ inline bool bar_of_row(const BarRect *__restrict__ rects, const int *__restrict__ rect_off, size_t pic, int yimg, int S, BarRect &r)
{
    const int r0 = rect_off[pic], n = rect_off[pic + 1] - r0;
    if (n < 1) return false;
    const int y = S - 1 - yimg;
    const double pitch = (double)S / (double)n;
    const int k0 = (int)floor(((double)y + 0.5) / pitch);
    for (int k = k0 - 1; k <= k0 + 1; k++) {
        if (k < 0 || k >= n) continue;
        const BarRect c = rects[r0 + k];
        if (y >= c.ya && y < c.yb) { r = c; return true; }
    }
    return false;
}

__global__ __launch_bounds__(OVL_THREADS) void barcode_kernel(const BarRect *__restrict__ rects, const int *__restrict__ rect_off, int n_pics, int S,
                                                              uint8_t *__restrict__ rgb, int vec_ok)
{
    const size_t rowb = (size_t)S * 3, per = rowb * S, total = per * n_pics, ngroups = (total + 15) / 16;
    for (size_t g = (size_t)blockIdx.x * OVL_THREADS + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * OVL_THREADS) {
        const size_t b0 = g * 16;
        const int cnt = total - b0 < 16 ? (int)(total - b0) : 16;
        size_t pic = b0 / per;
        const size_t rem = b0 - pic * per;
        int yimg = (int)(rem / rowb), cb = (int)(rem - (size_t)yimg * rowb);
        BarRect r;
        bool have = bar_of_row(rects, rect_off, pic, yimg, S, r);
        union { uint4 q; uint8_t b[16]; } o;
        for (int j = 0; j < cnt; j++) {
            const int x = cb / 3, ch = cb - 3 * x;
            o.b[j] = (have && x >= r.xa && x < r.xb) ? (uint8_t)((r.rgb >> (8 * ch)) & 255u) : (uint8_t)255;
            if (++cb == (int)rowb) {
                cb = 0;
                if (++yimg == S) { yimg = 0; pic++; }
                if (j + 1 < cnt) have = bar_of_row(rects, rect_off, pic, yimg, S, r);       // only then is (pic, yimg) still on the buffer
            }
        }
        if (cnt == 16 && vec_ok) *(uint4 *)(rgb + b0) = o.q;
        else for (int j = 0; j < cnt; j++) rgb[b0 + j] = o.b[j];
    }
}

}  // namespace

int barcode_render_dev(const BarRect *rects, const int *rect_off, int n_pics, int S, uint8_t *rgb, hipStream_t s)
{
    if (n_pics < 1 || S < 1 || (size_t)S * 3 > 0x7fffffffu) return -1;
    const size_t total = (size_t)S * S * 3 * n_pics, ngroups = (total + 15) / 16, blocks = (ngroups + OVL_THREADS - 1) / OVL_THREADS;
    const int vec_ok = ((uintptr_t)rgb & 15) == 0;
    hipLaunchKernelGGL(barcode_kernel, dim3((unsigned)std::min<size_t>(blocks, 65536)), dim3(OVL_THREADS), 0, s, rects, rect_off, n_pics, S, rgb, vec_ok);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int overlay_minmax_dev(const void *bg, int bg_dtype, int n, int bh, int bw, float *mnmx, hipStream_t s)
{
    // the ordered keys live behind the floats of the same buffer: mnmx must have room for 4 n words
    uint32_t *ord = (uint32_t *)(mnmx + 2 * (size_t)n);
    const size_t per = (size_t)bh * bw;
    const int chunks = (int)std::min<size_t>(64, (per + OVL_THREADS * 16 - 1) / (OVL_THREADS * 16));
    hipLaunchKernelGGL(ovl_minmax_init, dim3((n + 255) / 256), dim3(256), 0, s, ord, n);
    hipLaunchKernelGGL(ovl_minmax, dim3(chunks, n), dim3(OVL_THREADS), 0, s, bg, bg_dtype, per, ord);
    hipLaunchKernelGGL(ovl_minmax_finish, dim3((2 * n + 255) / 256), dim3(256), 0, s, ord, mnmx, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int overlay_render_dev(const void *bg, int bg_dtype, const float *mnmx, int n, int bh, int bw, const OverlaySeg *segs, const int *seg_offsets,
                       int vh, int vw, float rp, uint8_t *rgb, hipStream_t s)
{
    const dim3 grid((vw + OVL_TW - 1) / OVL_TW, (vh + OVL_TH - 1) / OVL_TH, n);
    if (grid.y > 65535u || grid.z > 65535u) return -1;
    hipLaunchKernelGGL(ovl_render, grid, dim3(OVL_THREADS), 0, s, bg, bg_dtype, mnmx, bh, bw, segs, seg_offsets, vh, vw, rp, rgb);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace tmat
