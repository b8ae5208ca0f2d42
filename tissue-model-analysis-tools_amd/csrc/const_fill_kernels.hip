// Constant-ring form of the down path (roi_plan.h:RoiDownPlan): the all-constant patches of a pass and the copies out of their tensors.
#include "tmat_internal.h"
#include "../../include/tmat.h"

#include <algorithm>
#include <vector>

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

// Shared-interior form (roi_plan.h:RoiDownPlan::share_fill).  Item blockIdx.y (uniform): every patch of the class takes the rectangle,
// all channels, from its neighbour nbr[3 patch + dir] -- right, below, diagonal -- at the position half a side to the left / above /
// both: the overlap of the two patches.  The source pixels are ones their patch computed and no item of the launch writes.
__global__ __launch_bounds__(256) void share_fill_kernel(float4 *t, const int *__restrict__ nbr, int H, int C4, const ShareItem *__restrict__ items)
{
    const ShareItem it = items[blockIdx.y];
    const size_t per = (size_t)H * H * C4;
    const int S = H / 2, dy = it.dir >= 1 ? S : 0, dx = it.dir != 1 ? S : 0;
    const long long total = (long long)it.np * it.rh * it.rw * C4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % C4);
        long long r = i / C4;
        const int x = it.x0 + (int)(r % it.rw);
        r /= it.rw;
        const int y = it.y0 + (int)(r % it.rh);
        const int p = it.p0 + (int)(r / it.rh);
        const int q = nbr[3 * p + it.dir];
        t[(size_t)p * per + ((size_t)y * H + x) * C4 + cq] = t[(size_t)q * per + ((size_t)(y - dy) * H + (x - dx)) * C4 + cq];
    }
}

// The launcher's checks (host tables): an item inside the tensor with its source rectangle, every source patch in range, and no source
// rectangle on a destination rectangle of the patch it is read from.
bool share_fill_check(int N, int H, int C, const int *nbr, const ShareItem *it, int n)
{
    if (n <= 0) return true;
    if (N <= 0 || H <= 0 || (H & 1) || C <= 0 || C % 4 != 0 || !nbr || !it || n > 65535) { set_error("launch_share_fill: bad argument"); return false; }
    const int S = H / 2;
    std::vector<unsigned char> from(n);        // from[j]: some patch of item i reads a patch of item j
    for (int i = 0; i < n; i++) {
        const ShareItem &q = it[i];
        const int dy = q.dir >= 1 ? S : 0, dx = q.dir != 1 ? S : 0;
        if (q.dir < 0 || q.dir > 2 || q.np <= 0 || q.p0 < 0 || q.p0 + q.np > N || q.rh <= 0 || q.rw <= 0 || q.y0 - dy < 0 || q.x0 - dx < 0 ||
            q.y0 + q.rh > H || q.x0 + q.rw > H) {
            set_error("launch_share_fill: an item leaves its tensor");
            return false;
        }
        std::fill(from.begin(), from.end(), 0);
        int last = -1;
        for (int p = q.p0; p < q.p0 + q.np; p++) {
            const int src = nbr[3 * p + q.dir];
            if (src < 0 || src >= N) { set_error("launch_share_fill: a source patch out of range"); return false; }
            if (last >= 0 && src >= it[last].p0 && src < it[last].p0 + it[last].np) continue;      // (the items of a class share p0 and np)
            for (int j = 0; j < n; j++)
                if (src >= it[j].p0 && src < it[j].p0 + it[j].np) { from[j] = 1; last = j; }
        }
        for (int j = 0; j < n; j++)
            if (from[j] && q.y0 - dy < it[j].y0 + it[j].rh && it[j].y0 < q.y0 - dy + q.rh && q.x0 - dx < it[j].x0 + it[j].rw && it[j].x0 < q.x0 - dx + q.rw) {
                set_error("launch_share_fill: a source rectangle overlaps a destination of its patch");
                return false;
            }
    }
    return true;
}

bool launch_share_fill(float *t, int N, int H, int C, const int *nbr_host, const int *nbr_dev, const ShareItem *it_host, const ShareItem *it_dev, int n,
                       hipStream_t s)
{
    if (n <= 0) return true;
    if (!nbr_dev || !it_dev) { set_error("launch_share_fill: bad argument"); return false; }
    if (!share_fill_check(N, H, C, nbr_host, it_host, n)) return false;
    long long most = 0;
    for (int i = 0; i < n; i++) most = std::max(most, (long long)it_host[i].np * it_host[i].rh * it_host[i].rw * (C / 4));
    const unsigned gx = (unsigned)std::min<long long>(1024, (most + 255) / 256);
    hipLaunchKernelGGL(share_fill_kernel, dim3(gx, n), dim3(256), 0, s, (float4 *)t, nbr_dev, H, C / 4, it_dev);
    return true;
}

}  // namespace tmat

extern "C" int tmat_debug_share_fill_check(int n_patches, int side, int channels, const int *neighbours, int n_items, const int *items)
{
    if (n_items < 0 || (n_items > 0 && !items)) { tmat::set_error("tmat_debug_share_fill_check: bad argument"); return TMAT_E_ARG; }
    std::vector<tmat::ShareItem> it(n_items);
    for (int i = 0; i < n_items; i++) {
        const int *q = items + (size_t)i * 7;
        it[i] = tmat::ShareItem{q[0], q[1], q[2], q[3], q[4], q[5], q[6]};
    }
    return tmat::share_fill_check(n_patches, side, channels, neighbours, it.data(), n_items) ? TMAT_OK : TMAT_E_ARG;
}
