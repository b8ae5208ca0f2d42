// Well detection (--detect-well): the superellipse fit of fl_tissue_model_tools/well_mask_generation.py on the device.
//
//   get_superellipse_hull (:16-91): of num_iters random candidates (t, d, s_a, s_b, c_x, c_y) keep those whose superellipse encloses
//   every hull point, max_k |u_k|^n + |v_k|^n < 1, and return the one of smallest area.  The candidates depend on (seed, num_iters)
//   alone: the host draws them and uploads, per candidate, c_x, c_y, cos t, sin t, d s_a, d s_b and the area (tmat_superellipse_table),
//   so the device evaluates no cos, sin or gamma.  One thread per candidate, the image's points in LDS, grid (blocks, images); the
//   smallest (area, index) comes out of a tree reduction per block and a second kernel over the blocks' results: no atomics decide it.
//   gen_superellipse_mask (:94-118): the same expression per pixel of a linspace(-1, 1) grid.
//
// Exactness.  The library is built with -ffp-contract=off: f64 subtraction, multiplication, division and addition give numpy's bits.
// n = 2: the reference squares (`** 2`), and so does the device: bit-identical, every candidate / pixel is decided here.
// n != 2: the reference calls pow; the device multiplies n - 1 times, which is within (n - 1) 2^-53 of the true power per term.  A
// value within SE_BAND = 1e-12 of 1 (> 1000 times that bound for n <= 64) is NOT decided here: its index goes to the band list and
// the caller evaluates it with the reference's own expression.
#include "../../include/tmat.h"
#include "tmat_ctx.h"

#include <algorithm>

namespace tmat {

#define SE_BLOCK 256
#define SE_MAX_PTS 1024
#define SE_MAX_EXP 64
#define SE_BAND 1e-12

// |a|^n by repeated multiplication, n >= 1
__device__ __forceinline__ double se_ipow(double a, int n)
{
    double p = a;
    for (int k = 1; k < n; k++) p = p * a;
    return p;
}

// the reference's value of candidate q = (c_x, c_y, cos t, sin t, d s_a, d s_b) at (x, y): the n == 2 branch of the SEARCH has no rotation
__device__ __forceinline__ double se_value_search(const double *q, double x, double y, int n)
{
    if (n == 2) {
        const double u = (x - q[0]) / q[4], v = (y - q[1]) / q[5];
        return u * u + v * v;
    }
    const double dx = x - q[0], dy = y - q[1];
    const double u = (dx * q[2] - dy * q[3]) / q[4], v = (dx * q[3] + dy * q[2]) / q[5];
    return se_ipow(fabs(u), n) + se_ipow(fabs(v), n);
}

struct SeBest { double area; int idx; };
__device__ __forceinline__ bool se_less(double a0, int i0, double a1, int i1)
{
    if (i0 < 0) return false;
    if (i1 < 0) return true;
    return a0 < a1 || (a0 == a1 && i0 < i1);
}

// grid (ceil(num_iters / SE_BLOCK), n_imgs).  partial[img][block] = the block's smallest (area, index) among the accepted candidates
__global__ __launch_bounds__(SE_BLOCK) void se_search_kernel(const double *__restrict__ table, int num_iters, const double *__restrict__ xy,
                                                            const int *__restrict__ offs, const int *__restrict__ n_exp,
                                                            SeBest *__restrict__ partial, int *__restrict__ band, int cap_band,
                                                            int *__restrict__ n_band)
{
    __shared__ double px[SE_MAX_PTS], py[SE_MAX_PTS];
    __shared__ double s_area[SE_BLOCK];
    __shared__ int s_idx[SE_BLOCK];
    const int img = blockIdx.y, p0 = offs[img];
    const int np = min(offs[img + 1] - p0, SE_MAX_PTS);      // the host has refused more
    const int n = n_exp[img];
    for (int k = threadIdx.x; k < np; k += SE_BLOCK) { px[k] = xy[2 * (size_t)(p0 + k)]; py[k] = xy[2 * (size_t)(p0 + k) + 1]; }
    __syncthreads();
    const int j = blockIdx.x * SE_BLOCK + threadIdx.x;
    double area = 0.0;
    int idx = -1;
    if (j < num_iters) {
        double q[7];
        for (int k = 0; k < 7; k++) q[k] = table[(size_t)j * 7 + k];
        double mx = -__builtin_inf();
        for (int k = 0; k < np; k++) {
            const double v = se_value_search(q, px[k], py[k], n);
            mx = v > mx ? v : mx;
        }
        bool accept;
        if (n == 2) accept = mx < 1.0;
        else {
            accept = mx < 1.0 - SE_BAND;
            if (!accept && !(mx > 1.0 + SE_BAND)) {             // undecided (a NaN lands here too): the caller evaluates it
                const int slot = atomicAdd(n_band, 1);
                if (slot < cap_band) { band[2 * slot] = img; band[2 * slot + 1] = j; }
            }
        }
        if (accept) { area = q[6]; idx = j; }
    }
    s_area[threadIdx.x] = area; s_idx[threadIdx.x] = idx;
    __syncthreads();
    for (int o = SE_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && se_less(s_area[threadIdx.x + o], s_idx[threadIdx.x + o], s_area[threadIdx.x], s_idx[threadIdx.x])) {
            s_area[threadIdx.x] = s_area[threadIdx.x + o]; s_idx[threadIdx.x] = s_idx[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)img * gridDim.x + blockIdx.x] = SeBest{s_area[0], s_idx[0]};
}

// one workgroup per image over its nblk partial results
__global__ __launch_bounds__(SE_BLOCK) void se_final_kernel(const SeBest *__restrict__ partial, int nblk, int *__restrict__ best)
{
    __shared__ double s_area[SE_BLOCK];
    __shared__ int s_idx[SE_BLOCK];
    const SeBest *p = partial + (size_t)blockIdx.x * nblk;
    double area = 0.0;
    int idx = -1;
    for (int k = threadIdx.x; k < nblk; k += SE_BLOCK)
        if (se_less(p[k].area, p[k].idx, area, idx)) { area = p[k].area; idx = p[k].idx; }
    s_area[threadIdx.x] = area; s_idx[threadIdx.x] = idx;
    __syncthreads();
    for (int o = SE_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && se_less(s_area[threadIdx.x + o], s_idx[threadIdx.x + o], s_area[threadIdx.x], s_idx[threadIdx.x])) {
            s_area[threadIdx.x] = s_area[threadIdx.x + o]; s_idx[threadIdx.x] = s_idx[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[blockIdx.x] = s_idx[0];
}

// gen_superellipse_mask: out[m][i][j] = |u|^n + |v|^n < 1 at x = xs[i], y = ys[j] (the orientation after the reference's swapaxes);
// the mask expression rotates for every n.  grid (blocks over H W, n_masks)
__global__ __launch_bounds__(SE_BLOCK) void se_mask_kernel(const double *__restrict__ params, const int *__restrict__ n_exp, const double *__restrict__ xs,
                                                          const double *__restrict__ ys, int H, int W, uint8_t *__restrict__ out,
                                                          long long *__restrict__ band, int cap_band, int *__restrict__ n_band)
{
    const int m = blockIdx.y, n = n_exp[m];
    const double *q = params + (size_t)m * 6;
    const double cx = q[0], cy = q[1], ct = q[2], st = q[3], da = q[4], db = q[5];
    const size_t npx = (size_t)H * W;
    for (size_t p = (size_t)blockIdx.x * SE_BLOCK + threadIdx.x; p < npx; p += (size_t)gridDim.x * SE_BLOCK) {
        const int i = (int)(p / W), j = (int)(p - (size_t)i * W);
        const double dx = xs[i] - cx, dy = ys[j] - cy;
        const double u = fabs((dx * ct - dy * st) / da), v = fabs((dx * st + dy * ct) / db);
        bool in;
        if (n == 2) in = u * u + v * v < 1.0;
        else {
            const double val = se_ipow(u, n) + se_ipow(v, n);
            in = val < 1.0 - SE_BAND;
            if (!in && !(val > 1.0 + SE_BAND)) {
                const int slot = atomicAdd(n_band, 1);
                if (slot < cap_band) band[slot] = (long long)((size_t)m * npx + p);
            }
        }
        out[(size_t)m * npx + p] = in;
    }
}

// skimage resize(order=0) as well_mask_generation.py:_resize_nearest has it: source index floor((i + 0.5) * (n_in / n_out)), f64
__global__ __launch_bounds__(SE_BLOCK) void se_resize_nearest_kernel(const uint8_t *__restrict__ in, int H, int W, int oh, int ow, uint8_t *__restrict__ out)
{
    const size_t onpx = (size_t)oh * ow;
    const double ry = (double)H / (double)oh, rx = (double)W / (double)ow;
    const uint8_t *src = in + (size_t)blockIdx.y * H * W;
    for (size_t p = (size_t)blockIdx.x * SE_BLOCK + threadIdx.x; p < onpx; p += (size_t)gridDim.x * SE_BLOCK) {
        const int i = (int)(p / ow), j = (int)(p - (size_t)i * ow);
        const int si = min((int)floor(((double)i + 0.5) * ry), H - 1), sj = min((int)floor(((double)j + 0.5) * rx), W - 1);
        out[(size_t)blockIdx.y * onpx + p] = src[(size_t)si * W + sj];
    }
}

static inline unsigned se_blocks(size_t n) { const size_t b = (n + SE_BLOCK - 1) / SE_BLOCK; return (unsigned)(b < 4096 ? (b ? b : 1) : 4096); }
void launch_resize_nearest_u8(const uint8_t *in, int n_img, int H, int W, int oh, int ow, uint8_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(se_resize_nearest_kernel, dim3(se_blocks((size_t)oh * ow), n_img), dim3(SE_BLOCK), 0, s, in, H, W, oh, ow, out);
}

// The two places the well mask enters the masked batch pipeline (pipeline.cpp; compute_branches.py:328, :334).
// img * well_mask on the rescaled image: x >= 0 there, so selecting +0.0f equals the reference's float32 * bool product bit for bit
__global__ __launch_bounds__(SE_BLOCK) void well_zero_kernel(float *__restrict__ x, const uint8_t *__restrict__ well, size_t n)
{
    for (size_t p = (size_t)blockIdx.x * SE_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * SE_BLOCK)
        if (!well[p]) x[p] = 0.0f;
}
// seg_mask * well_mask: (pred > 0.5) & well
__global__ __launch_bounds__(SE_BLOCK) void well_seg_kernel(const double *__restrict__ pred, const uint8_t *__restrict__ well, uint8_t *__restrict__ seg, size_t n)
{
    for (size_t p = (size_t)blockIdx.x * SE_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * SE_BLOCK)
        seg[p] = pred[p] > 0.5 && well[p];
}
void launch_well_zero_f32(float *x, const uint8_t *well, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(well_zero_kernel, dim3(se_blocks(n)), dim3(SE_BLOCK), 0, s, x, well, n);
}
void launch_well_seg(const double *pred, const uint8_t *well, uint8_t *seg, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(well_seg_kernel, dim3(se_blocks(n)), dim3(SE_BLOCK), 0, s, pred, well, seg, n);
}

}  // namespace tmat

using namespace tmat;

extern "C" {

int tmat_superellipse_table(tmat_handle hd, const double *table, int num_iters)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !table || num_iters < 1 || num_iters > (1 << 24)) { set_error("tmat_superellipse_table: bad argument"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    TMAT_HIP(hipStreamSynchronize(c->stream));              // nothing in flight reads the old table
    if (c->se_iters != num_iters) {
        if (c->se_table) hipFree(c->se_table);
        c->se_table = nullptr; c->se_iters = 0;
        TMAT_HIP(hipMalloc((void **)&c->se_table, (size_t)num_iters * 7 * sizeof(double)));
        c->se_iters = num_iters;
    }
    TMAT_HIP(hipMemcpy(c->se_table, table, (size_t)num_iters * 7 * sizeof(double), hipMemcpyHostToDevice));
    return TMAT_OK;
}

int tmat_superellipse_search(tmat_handle hd, const double *xy, const int *offs, int n_imgs, const int *n_exp, int *best, int *band_idx,
                             int cap_band, int *n_band)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !xy || !offs || !n_exp || !best || !n_band || n_imgs < 0 || cap_band < 0 || (cap_band > 0 && !band_idx)) {
        set_error("tmat_superellipse_search: bad argument");
        return TMAT_E_ARG;
    }
    *n_band = 0;
    if (n_imgs == 0) return TMAT_OK;
    if (!c->se_table) { set_error("tmat_superellipse_search: no candidate table on this handle (tmat_superellipse_table)"); return TMAT_E_ARG; }
    if (offs[0] != 0) { set_error("tmat_superellipse_search: offs[0] must be 0"); return TMAT_E_ARG; }
    for (int i = 0; i < n_imgs; i++) {
        const long long np = (long long)offs[i + 1] - offs[i];
        if (np < 1) { set_error("tmat_superellipse_search: every image needs at least one point"); return TMAT_E_ARG; }
        if (np > SE_MAX_PTS) { set_error("tmat_superellipse_search: more than 1024 points in one image"); return TMAT_E_CAP; }
        if (n_exp[i] < 1 || n_exp[i] > SE_MAX_EXP) { set_error("tmat_superellipse_search: exponent outside 1..64"); return TMAT_E_ARG; }
    }
    TMAT_HIP(hipSetDevice(c->device));
    const int nblk = (c->se_iters + SE_BLOCK - 1) / SE_BLOCK, npts = offs[n_imgs];
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    double *dxy = mem.alloc_from(xy, (size_t)npts * 2);
    int *doffs = mem.alloc_from(offs, (size_t)n_imgs + 1), *dn = mem.alloc_from(n_exp, n_imgs), *dbest = mem.alloc<int>(n_imgs);
    int *dband = mem.alloc<int>((size_t)std::max(cap_band, 1) * 2), *dcount = mem.alloc<int>(1);
    SeBest *partial = mem.alloc<SeBest>((size_t)n_imgs * nblk);
    if (!mem.ok || !mem.check(hipMemsetAsync(dcount, 0, sizeof(int), s), "memset")) return TMAT_E_HIP;
    hipLaunchKernelGGL(se_search_kernel, dim3(nblk, n_imgs), dim3(SE_BLOCK), 0, s, c->se_table, c->se_iters, dxy, doffs, dn, partial, dband, cap_band, dcount);
    hipLaunchKernelGGL(se_final_kernel, dim3(n_imgs), dim3(SE_BLOCK), 0, s, partial, nblk, dbest);
    int *hcount = mem.host<int>();
    mem.check(hipGetLastError(), "superellipse search launch");
    mem.d2h(best, dbest, (size_t)n_imgs * sizeof(int));
    mem.d2h(hcount, dcount, sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    const int count = *n_band = *hcount;
    if (count > cap_band) { set_error("tmat_superellipse_search: more undecided candidates than cap_band"); return TMAT_E_CAP; }
    if (count > 0) {
        if (!mem.check(hipMemcpy(band_idx, dband, (size_t)count * 2 * sizeof(int), hipMemcpyDeviceToHost), "D2H")) return TMAT_E_HIP;
        // the slots were taken in arrival order: (image, candidate) ascending for the caller
        struct Pair { int img, cand; };
        Pair *pr = (Pair *)band_idx;
        std::sort(pr, pr + count, [](const Pair &a, const Pair &b) { return a.img != b.img ? a.img < b.img : a.cand < b.cand; });
    }
    return TMAT_OK;
}

int tmat_superellipse_masks(tmat_handle hd, const double *params, int n_masks, const int *n_exp, const double *xs, const double *ys, int H, int W,
                            uint8_t *out, long long *band_px, int cap_band, int *n_band)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !params || !n_exp || !xs || !ys || !out || !n_band || n_masks < 0 || H < 1 || W < 1 || cap_band < 0 || (cap_band > 0 && !band_px)) {
        set_error("tmat_superellipse_masks: bad argument");
        return TMAT_E_ARG;
    }
    *n_band = 0;
    if (n_masks == 0) return TMAT_OK;
    for (int i = 0; i < n_masks; i++)
        if (n_exp[i] < 1 || n_exp[i] > SE_MAX_EXP) { set_error("tmat_superellipse_masks: exponent outside 1..64"); return TMAT_E_ARG; }
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)H * W;
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    double *dpar = mem.alloc_from(params, (size_t)n_masks * 6), *dxs = mem.alloc_from(xs, H), *dys = mem.alloc_from(ys, W);
    int *dn = mem.alloc_from(n_exp, n_masks), *dcount = mem.alloc<int>(1);
    long long *dband = mem.alloc<long long>(std::max(cap_band, 1));
    uint8_t *dout = mem.alloc<uint8_t>((size_t)n_masks * npx);
    if (!mem.ok || !mem.check(hipMemsetAsync(dcount, 0, sizeof(int), s), "memset")) return TMAT_E_HIP;
    hipLaunchKernelGGL(se_mask_kernel, dim3(se_blocks(npx), n_masks), dim3(SE_BLOCK), 0, s, dpar, dn, dxs, dys, H, W, dout, dband, cap_band, dcount);
    int *hcount = mem.host<int>();
    mem.check(hipGetLastError(), "superellipse mask launch");
    mem.d2h(out, dout, (size_t)n_masks * npx);
    mem.d2h(hcount, dcount, sizeof(int));
    if (mem.finish()) return TMAT_E_HIP;
    const int count = *n_band = *hcount;
    if (count > cap_band) { set_error("tmat_superellipse_masks: more undecided pixels than cap_band"); return TMAT_E_CAP; }
    if (count > 0) {
        if (!mem.check(hipMemcpy(band_px, dband, (size_t)count * sizeof(long long), hipMemcpyDeviceToHost), "D2H")) return TMAT_E_HIP;
        std::sort(band_px, band_px + count);
    }
    return TMAT_OK;
}

int tmat_resize_nearest_u8(tmat_handle hd, const uint8_t *in, int n, int H, int W, int out_h, int out_w, uint8_t *out)
{
    Ctx *c = (Ctx *)hd;
    if (!c || !in || !out || n < 0 || H < 1 || W < 1 || out_h < 1 || out_w < 1) { set_error("tmat_resize_nearest_u8: bad argument"); return TMAT_E_ARG; }
    if (n == 0) return TMAT_OK;
    TMAT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)H * W, onpx = (size_t)out_h * out_w;
    hipStream_t s = c->stream;
    DevScope mem(c->ws_pool, s);
    uint8_t *din = mem.alloc_from(in, (size_t)n * npx), *dout = mem.alloc<uint8_t>((size_t)n * onpx);
    if (!mem.ok) return TMAT_E_HIP;
    hipLaunchKernelGGL(se_resize_nearest_kernel, dim3(se_blocks(onpx), n), dim3(SE_BLOCK), 0, s, din, H, W, out_h, out_w, dout);
    mem.check(hipGetLastError(), "nearest resize launch");
    mem.d2h(out, dout, (size_t)n * onpx);
    return mem.finish();
}

}  // extern "C"
