// Constant-ring form of the down path (roi_plan.h:RoiDownPlan): the all-constant patches of a pass and the copies out of their tensors.
#include "tmat_internal.h"
#include "../../include/tmat.h"

#include <algorithm>

namespace tmat {

// patch blockIdx.y of out (k, pp4 float4): padval[blockIdx.y] everywhere
__global__ __launch_bounds__(256) void const_patch_kernel(const float *__restrict__ padval, int pp4, float4 *__restrict__ out)
{
    const float v = padval[blockIdx.y];
    float4 *o = out + (size_t)blockIdx.y * pp4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < pp4; i += gridDim.x * 256) o[i] = make_float4(v, v, v, v);
}

void launch_const_patches(const float *padval, int k, int pp, float *out, hipStream_t s)
{
    if (k <= 0) return;
    const int pp4 = pp / 4;
    hipLaunchKernelGGL(const_patch_kernel, dim3(std::min(64, (pp4 + 255) / 256), k), dim3(256), 0, s, padval, pp4, (float4 *)out);
}

// Item blockIdx.y (uniform: the table is read with scalar loads): every patch of the class takes the strip, all channels, from the
// all-constant patch of its image at the same position.  Source and destination are different patches of the same tensor.
__global__ __launch_bounds__(256) void const_fill_kernel(float4 *t, int src0, int H, int C4, FillItems f)
{
    const FillItem it = f.it[blockIdx.y];
    const size_t per = (size_t)H * H * C4;
    const long long total = (long long)it.np * it.rh * it.rw * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % C4);
        long long r = i / C4;
        const int x = it.x0 + (int)(r % it.rw);
        r /= it.rw;
        const int y = it.y0 + (int)(r % it.rh);
        const int p = (int)(r / it.rh);
        const size_t at = ((size_t)y * H + x) * C4 + cq;
        t[(size_t)(it.p0 + p) * per + at] = t[(size_t)(src0 + p / it.cnt) * per + at];
    }
}

bool launch_const_fill(float *t, int src0, int N, int H, int C, const FillItems &f, hipStream_t s)
{
    if (f.n <= 0) return true;
    long long most = 0;
    bool ok = f.n <= 64 && C > 0 && C % 4 == 0 && src0 >= 0 && src0 <= N;
    for (int i = 0; ok && i < f.n; i++) {
        const FillItem &q = f.it[i];
        ok = q.np > 0 && q.cnt > 0 && q.np % q.cnt == 0 && q.p0 >= 0 && q.p0 + q.np <= src0 && src0 + q.np / q.cnt <= N &&
             q.rh > 0 && q.rw > 0 && q.y0 >= 0 && q.x0 >= 0 && q.y0 + q.rh <= H && q.x0 + q.rw <= H;
        most = std::max(most, (long long)q.np * q.rh * q.rw * (C / 4));
    }
    if (!ok) { set_error("launch_const_fill: a strip leaves its tensor"); return false; }
    const unsigned gx = (unsigned)std::min<long long>(2048, (most + 255) / 256);
    hipLaunchKernelGGL(const_fill_kernel, dim3(gx, f.n), dim3(256), 0, s, (float4 *)t, src0, H, C / 4, f);
    return true;
}

}  // namespace tmat
