// Stage pictures on gfx950: save_vis (compute_branches.py:74-78 = rescale_intensity(out_range=(0, 255)) + cv2.imwrite's cast) of a
// batch of images that are already in HBM -- original_image.png (:315), prediction.png (:331), segmentation_mask.png (:347),
// distance_transform.png (:348), and the two pictures of the Z-stack branch (:228-229, :303).  Per image, in f64, in this order:
//   lo, hi = min / max over the non-NaN values
//   v = hi != lo ? ((a - lo) / (hi - lo)) * 255 : min(max(a, 0), 255);  NaN -> 0;  out = (u8) rint(v), ties to even
// An image that is all NaN has lo = hi = NaN here and comes out all zero.  Infinities are outside the contract (include/tmat.h).
//   vis_minmax_partial / vis_minmax_final   NaN-ignoring extrema: up to 64 workgroups per image reduce in the wave, then in LDS, and
//                                           write one partial pair each; a second tiny kernel folds them.  Min and max do not depend on
//                                           the order, so the result does not depend on scheduling.
//   vis_picture_kernel                      HBM-bound streaming kernel, grid (blocks, images): a thread takes 16 consecutive pixels with
//                                           16-byte loads and writes them with one 16-byte store.  The 16-pixel groups are aligned on the
//                                           FLAT index of the batch (image * per + pixel), which aligns input and output of every type
//                                           at once; the pixels of an image in front of its first and behind its last whole group are
//                                           done one by one.  No LDS.
// The host twin is vis_pictures_host (postproc.cpp): the same bytes.
#include "../../include/tmat.h"
#include "tmat_internal.h"
#include "morph.h"

#include <cmath>

namespace tmat {
namespace {

constexpr int VIS_THREADS = 256, VIS_MAX_CHUNKS = 64;

template <typename T>
__global__ __launch_bounds__(VIS_THREADS) void vis_minmax_partial(const T *__restrict__ a, size_t per, double *__restrict__ part)
{
    const T *p = a + (size_t)blockIdx.y * per;
    double lo = INFINITY, hi = -INFINITY;           // a NaN fails both comparisons and is skipped
    for (size_t i = (size_t)blockIdx.x * VIS_THREADS + threadIdx.x; i < per; i += (size_t)gridDim.x * VIS_THREADS) {
        const double v = (double)p[i];
        lo = v < lo ? v : lo; hi = v > hi ? v : hi;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double l2 = __shfl_down(lo, o), h2 = __shfl_down(hi, o);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    __shared__ double slo[VIS_THREADS / 64], shi[VIS_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < VIS_THREADS / 64; i++) { lo = slo[i] < lo ? slo[i] : lo; hi = shi[i] > hi ? shi[i] : hi; }
        double *dst = part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        dst[0] = lo; dst[1] = hi;
    }
}

__global__ void vis_minmax_final(const double *__restrict__ part, int chunks, int k, double *__restrict__ lo_out, double *__restrict__ hi_out)
{
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= k) return;
    double lo = INFINITY, hi = -INFINITY;
    for (int j = 0; j < chunks; j++) {
        const double l2 = part[2 * ((size_t)img * chunks + j)], h2 = part[2 * ((size_t)img * chunks + j) + 1];
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if (lo > hi) lo = hi = NAN;         // no value that is not NaN: np.nanmin / np.nanmax give NaN
    lo_out[img] = lo; hi_out[img] = hi;
}

__device__ __forceinline__ uint8_t vis_px(double a, double lo, double hi, bool scale)
{
    double v = scale ? ((a - lo) / (hi - lo)) * 255.0 : fmin(fmax(a, 0.0), 255.0);
    if (!(v == v)) v = 0.0;             // np.nan_to_num
    return (uint8_t)(int)rint(v);
}

// E: the type the extrema are held in -- double (vis_minmax_final, finish_dev's lo / hi) or int (launch_rescale01's mn / mx)
template <typename T, typename E>
__global__ __launch_bounds__(VIS_THREADS) void vis_picture_kernel(const T *__restrict__ a, size_t per, const E *__restrict__ lov,
                                                                  const E *__restrict__ hiv, uint8_t *__restrict__ out, int vec_ok)
{
    const int img = blockIdx.y;
    const double lo = (double)lov[img], hi = (double)hiv[img];
    const bool scale = hi != lo;
    const size_t g0 = (size_t)img * per, g1 = g0 + per;                     // the image's flat pixel range
    size_t a0 = (g0 + 15) & ~(size_t)15;                                    // its first whole group of 16
    if (!vec_ok || a0 > g1) a0 = g1;
    const size_t nch = (g1 - a0) / 16, a1 = a0 + nch * 16;
    const size_t t = (size_t)blockIdx.x * VIS_THREADS + threadIdx.x, stride = (size_t)gridDim.x * VIS_THREADS;
    for (size_t c = t; c < nch; c += stride) {
        union { uint4 q[sizeof(T)]; T e[16]; } in;
        const uint4 *src = (const uint4 *)(a + a0 + c * 16);
#pragma unroll
        for (int j = 0; j < (int)sizeof(T); j++) in.q[j] = src[j];
        union { uint4 q; uint8_t b[16]; } o;
#pragma unroll
        for (int j = 0; j < 16; j++) o.b[j] = vis_px((double)in.e[j], lo, hi, scale);
        *(uint4 *)(out + a0 + c * 16) = o.q;
    }
    const size_t nh = a0 - g0, ns = nh + (g1 - a1);                         // [g0, a0) and [a1, g1), one pixel per thread
    for (size_t i = t; i < ns; i += stride) {
        const size_t g = i < nh ? g0 + i : a1 + (i - nh);
        out[g] = vis_px((double)a[g], lo, hi, scale);
    }
}

template <typename T, typename E>
int launch_picture(const void *a, int k, size_t per, const E *lo, const E *hi, uint8_t *out, hipStream_t s)
{
    if (k < 1 || k > 65535 || per < 1) return -1;
    const int vec_ok = ((uintptr_t)a & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const size_t groups = (per + 16 * VIS_THREADS - 1) / (16 * VIS_THREADS);
    const dim3 grid((unsigned)(groups < 1024 ? groups : 1024), k);
    hipLaunchKernelGGL((vis_picture_kernel<T, E>), grid, dim3(VIS_THREADS), 0, s, (const T *)a, per, lo, hi, out, vec_ok);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int minmax_chunks(size_t per)
{
    const size_t c = (per + 16 * VIS_THREADS - 1) / (16 * VIS_THREADS);
    return (int)(c < (size_t)VIS_MAX_CHUNKS ? c : (size_t)VIS_MAX_CHUNKS);
}

}  // namespace

size_t vis_scratch_bytes(int k) { return (size_t)k * (2 * VIS_MAX_CHUNKS + 2) * sizeof(double); }

// lo / hi (k doubles each) of vis_scratch: where vis_minmax_dev leaves the extrema
double *vis_scratch_lo(void *scratch, int k) { return (double *)scratch + (size_t)k * 2 * VIS_MAX_CHUNKS; }

// a (k, per) of dtype (TMAT_PIC_*) on the device -> per-image NaN-ignoring extrema in vis_scratch_lo(scratch, k)[0..k) and [k..2k)
int vis_minmax_dev(const void *a, int dtype, int k, size_t per, void *scratch, hipStream_t s)
{
    if (k < 1 || k > 65535 || per < 1) return -1;
    double *part = (double *)scratch, *lo = vis_scratch_lo(scratch, k), *hi = lo + k;
    const int chunks = minmax_chunks(per);
    const dim3 grid(chunks, k), blk(VIS_THREADS);
    switch (dtype) {
    case TMAT_PIC_U16: hipLaunchKernelGGL((vis_minmax_partial<uint16_t>), grid, blk, 0, s, (const uint16_t *)a, per, part); break;
    case TMAT_PIC_F32: hipLaunchKernelGGL((vis_minmax_partial<float>), grid, blk, 0, s, (const float *)a, per, part); break;
    case TMAT_PIC_F64: hipLaunchKernelGGL((vis_minmax_partial<double>), grid, blk, 0, s, (const double *)a, per, part); break;
    case TMAT_PIC_U8: hipLaunchKernelGGL((vis_minmax_partial<uint8_t>), grid, blk, 0, s, (const uint8_t *)a, per, part); break;
    default: return -1;
    }
    hipLaunchKernelGGL(vis_minmax_final, dim3((k + 255) / 256), dim3(256), 0, s, part, chunks, k, lo, hi);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// a (k, per) of dtype on the device, extrema lo / hi (k doubles, device) -> out (k, per) u8 on the device
int vis_picture_dev(const void *a, int dtype, int k, size_t per, const double *lo, const double *hi, uint8_t *out, hipStream_t s)
{
    switch (dtype) {
    case TMAT_PIC_U16: return launch_picture<uint16_t, double>(a, k, per, lo, hi, out, s);
    case TMAT_PIC_F32: return launch_picture<float, double>(a, k, per, lo, hi, out, s);
    case TMAT_PIC_F64: return launch_picture<double, double>(a, k, per, lo, hi, out, s);
    case TMAT_PIC_U8: return launch_picture<uint8_t, double>(a, k, per, lo, hi, out, s);
    default: return -1;
    }
}

// the u16 image with the integer extrema launch_rescale01 has already found (PassBuf::mn / mx)
int vis_picture_u16_dev(const uint16_t *a, int k, size_t per, const int *mn, const int *mx, uint8_t *out, hipStream_t s)
{
    return launch_picture<uint16_t, int>(a, k, per, mn, mx, out, s);
}

}  // namespace tmat
