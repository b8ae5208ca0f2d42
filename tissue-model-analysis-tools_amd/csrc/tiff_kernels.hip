// TIFF decoder on the device (tiff.h).  Two kernels per chunk of planes, on one stream:
//   tiff_strips_kernel   one workgroup of one wave per strip, all strips of all planes of the chunk in one grid.  LZW and PackBits are
//                        serial per strip: lane 0 runs tiff_strip_decode (the host twin's function) with the 16 KiB string table in LDS
//                        and writes the strip's raw bytes; the other lanes leave at once.  Uncompressed strips leave at once too: their
//                        rows are read in place.
//   tiff_rows_kernel     one workgroup per row: byte order, predictor 2 as a block-wide running sum, widening to uint16.
// No workgroup waits for another and nothing spins.  A corrupt strip sets its plane's flag; the rows kernel, which starts after the
// strips kernel has finished, skips such a plane, so its output slice is not written.
#include "tiff.h"

namespace tmat {

constexpr int TIFF_ROW_THREADS = 256;

__global__ __launch_bounds__(64) void tiff_strips_kernel(const uint8_t *__restrict__ blob, const TiffStrip *__restrict__ strips, int n_strips,
                                                         const TiffPlane *__restrict__ planes, uint8_t *__restrict__ raw, int *__restrict__ bad)
{
    __shared__ uint32_t table[TIFF_LZW_SIZE];
    const int i = (int)blockIdx.x;
    if (i >= n_strips || threadIdx.x != 0) return;
    const TiffStrip s = strips[i];
    if (s.comp == TIFF_COMP_NONE) return;
    const TiffPlane &p = planes[s.plane];
    if (tiff_strip_decode(s.comp, blob + p.file_base + s.src, s.n_in, raw + p.raw + s.dst, s.n_out, table) != TIFF_OK) bad[s.plane] = 1;
}

__global__ __launch_bounds__(TIFF_ROW_THREADS) void tiff_rows_kernel(const uint8_t *__restrict__ blob, const TiffStrip *__restrict__ strips,
                                                                     const TiffPlane *__restrict__ planes, int H, int W,
                                                                     const uint8_t *__restrict__ raw, uint16_t *__restrict__ out,
                                                                     const int *__restrict__ bad)
{
    __shared__ uint32_t part[TIFF_ROW_THREADS];
    const int y = (int)blockIdx.x, pi = (int)blockIdx.y, t = (int)threadIdx.x;
    const TiffPlane p = planes[pi];
    if (!p.ok || bad[pi]) return;                           // uniform over the workgroup
    const uint8_t *row = tiff_row(p, strips, blob + p.file_base, raw + p.raw, y, W);
    uint16_t *o = out + ((size_t)p.out_index * H + y) * (size_t)W;
    if (p.predictor != 2) {
        for (int x = t; x < W; x += TIFF_ROW_THREADS) o[x] = tiff_widen(tiff_sample(row, x, p.bytes, p.swap), p.bytes);
        return;
    }
    // running sum: each thread owns `per` consecutive samples; the sums of the threads before it come from a scan in LDS
    const int per = (W + TIFF_ROW_THREADS - 1) / TIFF_ROW_THREADS;
    const int x0 = min(t * per, W), x1 = min(x0 + per, W);
    uint32_t sum = 0;
    for (int x = x0; x < x1; x++) sum += tiff_sample(row, x, p.bytes, p.swap);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < TIFF_ROW_THREADS; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t acc = part[t] - sum;                           // exclusive prefix; modulo 2^32, and so modulo 2^bits
    for (int x = x0; x < x1; x++) {
        acc += tiff_sample(row, x, p.bytes, p.swap);
        o[x] = tiff_widen(acc, p.bytes);
    }
}

int tiff_decode_launch(const uint8_t *blob, const TiffStrip *strips, int n_strips, const TiffPlane *planes, int n_planes, int H, int W,
                       uint8_t *raw, uint16_t *out, int *bad, hipStream_t s)
{
    if (n_planes < 1 || n_planes > 65535 || n_strips < 0) return 1;
    if (hipMemsetAsync(bad, 0, (size_t)n_planes * sizeof(int), s) != hipSuccess) return 1;
    if (n_strips > 0) {
        hipLaunchKernelGGL(tiff_strips_kernel, dim3((unsigned)n_strips), dim3(64), 0, s, blob, strips, n_strips, planes, raw, bad);
        if (hipGetLastError() != hipSuccess) return 1;
        hipLaunchKernelGGL(tiff_rows_kernel, dim3((unsigned)H, (unsigned)n_planes), dim3(TIFF_ROW_THREADS), 0, s, blob, strips, planes, H, W,
                           raw, out, bad);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    return 0;
}

}  // namespace tmat
