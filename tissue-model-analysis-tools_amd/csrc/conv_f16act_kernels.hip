// Convolution of the invasion-depth classifier's "f16act" mode (TMAT_RESNET_PRECISION_F16ACT, include/tmat.h): activations
// live in memory as IEEE binary16.  Implicit GEMM on v_mfma_f32_32x32x16_f16 like PREC = 3 of conv_mfma_kernel (unet_kernels.hip), with
// the same k-step geometry -- a k step is 16 consecutive channels of one tap, lane half h carries channels 8 h .. 8 h + 7 of them, an
// accumulator takes its k steps in the order (32-channel block, tap, k step) ascending -- so on f16-exact operands the accumulators are
// those of PREC = 3 bit for bit.  What differs is everything around the matrix instruction:
//   * the A tile is f16 in memory: LDS-DMA'd as 64-byte rows (32 channels), no conversion and no clamp in the K loop -- a lane's
//     fragment of a k step is ONE ds_read_b128 = 8 halves = one MFMA operand;
//   * the epilogue is the f32 code of every form (fmaf(acc, scale, shift), + residual, ReLU), the residual read as f16 and widened
//     (exact), the result rounded ONCE to f16 (nearest even, beyond +-65504 saturating: v_med3_f32 in front of v_cvt_f16_f32) and stored
//     as 16-byte rows of 8 channels.
// LDS layout of one stage: BM A rows then BN weight rows, 64 bytes each; the 16-byte unit u (channels 8 u .. 8 u + 7) of row r sits in
// slot u ^ ((r >> 2) & 3).  The DMA destination is lane-linear (a wave fills 16 rows), so the swizzle is applied to the per-lane SOURCE
// address.  Bank argument: a ds_read_b128 is served in 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32); lane l reads row
// base + (l & 31), and 256 bytes = 4 rows span the 64 banks, so a row's 16-byte bank group is 4 (r & 3) + slot.  The rows of a group are
// four runs of four consecutive rows with four different keys (r >> 2) & 3 -- {0, 3, 1, 2} and {1, 2, 0, 3} -- so for each r & 3 the four
// rows read four different slots: 16 distinct bank groups, conflict-free.  (The weight planes of PREC = 1 .. 3 use the same rows.)
// 32 channels per chunk and barrier, not 64: with 3 x 3 taps the contract's order walks all nine taps of a 32-channel block before the
// next block, so a 64-channel chunk would reorder the accumulation; and Cin = 64, K = 192 would give odd chunk counts.
#include "dev_guard.h"
#include "tmat_internal.h"
#include "../../include/tmat.h"

namespace tmat {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;

// exact division of 0 <= n < 2^31 by a launch constant d >= 2 (the construction of unet_kernels.hip:FastDiv)
struct FDiv {
    unsigned mul;
    int sh;
};
FDiv make_fdiv(int d)
{
    int l = 0;
    while ((1ll << l) < d) l++;
    const unsigned long long num = 1ull << (31 + l);
    return FDiv{(unsigned)((num + (unsigned long long)d - 1) / (unsigned long long)d), l - 1};
}
__device__ __forceinline__ int fdiv(int n, FDiv f) { return (int)(__umulhi((unsigned)n, f.mul) >> f.sh); }

__device__ __forceinline__ _Float16 f16_sat(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }

// 8 waves as WM x WN, each owning (BM / WM) x (BN / WN) outputs as TM x TN tiles of 32 x 32; 4 waves per SIMD (128 registers), two
// workgroups per CU (the epilogue's slabs make a workgroup 64 KiB of LDS at 128 x 128 and 256 x 64)
template <int BM, int BN, int WM, int WN, int KS>
__global__ __launch_bounds__(512, 4) void conv_f16act_kernel(ConvF16Args a, int M, int Ho, int Wo, int nMt, int nNt, FDiv dHW, FDiv dW)
{
    static_assert(WM * WN == 8, "8 waves");
    constexpr int NT = 512;
    constexpr int RB = 64;                           // bytes per LDS row: 32 halves
    constexpr int RP = NT / 4;                       // rows per DMA pass: 4 lanes x 16 B per row
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NPA = BM / RP;
    static_assert(NPA >= 1 && NPA * RP == BM && BN <= RP && BN % 16 == 0 && TM >= 1 && TN >= 1, "tile");
    constexpr int taps = KS * KS;
    // bytes per stage: the operand rows, and at least half of the epilogue's eight wave-private f32 slabs
    constexpr int STAGE = (BM + BN) * RB > BM * BN * 2 ? (BM + BN) * RB : BM * BN * 2;
    // one LDS object per stage: the DMA in flight into one stage does not alias the reads of the other (see conv_mfma_kernel)
    __shared__ __attribute__((aligned(16))) char stage0[STAGE];
    __shared__ __attribute__((aligned(16))) char stage1[STAGE];

    // blocks b and b + 8 share an XCD: the nNt column tiles of one pixel tile go to the same XCD, whose L2 serves the re-read A rows
    const int b = blockIdx.x;
    const int xcd = b & 7, j = b >> 3;
    const int nt = j % nNt, mt = (j / nNt) * 8 + xcd;
    if (mt >= nMt) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int HW = Ho * Wo;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;

    auto stored_pixel = [&](int m) {      // linear index of the stored pixel that output pixel m is centred on
        const int n = fdiv(m, dHW);
        const int r = m - n * HW;
        const int y = fdiv(r, dW);
        const int x = r - y * Wo;
        return (n * a.h + y * a.stride) * a.w + x * a.stride;
    };
    // DMA role: row t >> 2 of every pass, slot t & 3, i.e. channels 8 u .. 8 u + 7 with u = (t & 3) ^ ((row >> 2) & 3).  The A buffer
    // starts (w + 1) stored pixels before the tile's first one; a lane's voffset is its pixel's distance from that first pixel and the
    // tap / channel-block displacement is the scalar soffset.  Taps outside the image and rows past M get a voffset beyond num_records:
    // the range check returns zeros.
    const int srow = t >> 2;
    const int c8 = ((t & 3) ^ ((srow >> 2) & 3)) * 8;
    constexpr unsigned OOB = 0x80000000u;
    const int p0 = __builtin_amdgcn_readfirstlane(stored_pixel(m0));
    unsigned pvt[taps][NPA];
#pragma unroll
    for (int i = 0; i < NPA; i++) {
        const int m = m0 + i * RP + srow;
        const bool ok = m < M;
        const int mm = ok ? m : m0;
        const int n = fdiv(mm, dHW);
        const int r = mm - n * HW;
        const int yo = fdiv(r, dW);
        const int y = yo * a.stride, x = (r - yo * Wo) * a.stride;
        const unsigned pv = (unsigned)(((n * a.h + y) * a.w + x - p0) * a.Cin + c8) * 2u;
        unsigned msk = 1u;          // bit ky * 3 + kx: row y + ky - 1 and column x + kx - 1 lie inside the image
        if (KS == 3) {
            const unsigned ym = (y > 0 ? 0x007u : 0u) | 0x038u | (y + 1 < a.h ? 0x1C0u : 0u);
            const unsigned xm = (x > 0 ? 0x049u : 0u) | 0x092u | (x + 1 < a.w ? 0x124u : 0u);
            msk = ym & xm;
        }
        if (!ok) msk = 0u;
#pragma unroll
        for (int tp = 0; tp < taps; tp++) pvt[tp][i] = ((msk >> tp) & 1u) ? pv : OOB;
    }
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)(a.in + ((long)p0 - a.w - 1) * a.Cin), 0, 0x7fffffff, 0x00020000);
    // weights [tap][Cout][Cin]: row n0 + srow (the waves that hold one: 16 rows each), this lane's channel group
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void *)(a.W + (size_t)n0 * a.Cin), 0, 0x7fffffff, 0x00020000);
    const unsigned wv = (unsigned)(srow * a.Cin + c8) * 2u;
    const int wtap = a.Cout * a.Cin * 2;             // bytes per tap
    const int ldsw = wave * 16 * RB;                 // this wave's 16 rows inside a pass

    // chunk (tap T_, channel block cb_) into stage st_: T_ is a compile-time constant at every use (the K loop is unrolled over the taps)
#define F16A_ISSUE(st_, T_, cb_)                                                                                   \
    {                                                                                                              \
        const int soA_ = ((KS == 3 ? ((T_) / 3) * a.w + (T_) % 3 : a.w + 1) * a.Cin + (cb_) * 32) * 2;             \
        const int soB_ = (T_) * wtap + (cb_) * 64;                                                                 \
        _Pragma("unroll") for (int i = 0; i < NPA; i++) {                                                          \
            const unsigned vo_ = pvt[T_][i];                                                                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t *)((st_) + i * RP * RB + ldsw), 16, vo_, soA_, 0, 0); \
        }                                                                                                          \
        if (wave * 16 < BN)                                                                                        \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t *)((st_) + BM * RB + ldsw), 16, wv, soB_, 0, 0); \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int jn = 0; jn < TN; jn++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][jn][r] = 0.f;

    // fragments: row = tile base + (lane & 31) (bases are multiples of 32, so the key is (lane >> 2) & 3); k step tk = channels
    // 16 tk .. 16 tk + 15, of which this lane half carries 8 hi .. 8 hi + 7: unit 2 tk + hi
    const int hi = lane >> 5, key = (lane >> 2) & 3;
    const int arow = (wm * (BM / WM) + (lane & 31)) * RB;
    const int brow = (BM + wn * (BN / WN) + (lane & 31)) * RB;

    // one step = one chunk: all its fragments (2 TM + 2 TN ds_read_b128), the next chunk's DMA into the other stage, 2 TM TN MFMAs, then
    // the wave retires its own DMA and the workgroup meets at the barrier (data order of LDS-DMA: that wait, then the barrier)
#define F16A_STEP(cur_, nxt_, more_, T_, cb_)                                                                      \
    {                                                                                                              \
        f16x8 af[2][TM], bf[2][TN];                                                                                \
        _Pragma("unroll") for (int tk = 0; tk < 2; tk++) {                                                         \
            const int slot = ((2 * tk + hi) ^ key) * 16;                                                           \
            _Pragma("unroll") for (int i = 0; i < TM; i++) af[tk][i] = *reinterpret_cast<const f16x8 *>((cur_) + arow + i * 32 * RB + slot); \
            _Pragma("unroll") for (int jn = 0; jn < TN; jn++) bf[tk][jn] = *reinterpret_cast<const f16x8 *>((cur_) + brow + jn * 32 * RB + slot); \
        }                                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        if (more_) F16A_ISSUE(nxt_, T_, cb_)                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        _Pragma("unroll") for (int tk = 0; tk < 2; tk++)                                                           \
            _Pragma("unroll") for (int i = 0; i < TM; i++)                                                         \
                _Pragma("unroll") for (int jn = 0; jn < TN; jn++)                                                  \
                    acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[tk][i], bf[tk][jn], acc[i][jn], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                           \
        __syncthreads();                                                                                           \
    }

    F16A_ISSUE(stage0, 0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // chunk c = (channel block c / taps, tap c % taps); even chunks live in stage0.  The body is UNR chunks, unrolled: UNR is the smallest
    // even multiple of the tap count (the host checks that Cin / 32 is even), so chunk c + u has stage u & 1 and the chunk loaded in its
    // step has tap (u + 1) % taps and channel block cb + (u + 1) / taps, both known at compile time relative to cb.
    constexpr int UNR = (taps & 1) ? 2 * taps : taps;
    const int nchunks = taps * (a.Cin / 32);
    for (int c = 0, cb = 0; c < nchunks; c += UNR, cb += UNR / taps) {
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const bool more = u + 1 < UNR || c + UNR < nchunks;
            if (u & 1) F16A_STEP(stage1, stage0, more, (u + 1) % taps, cb + (u + 1) / taps)
            else F16A_STEP(stage0, stage1, more, (u + 1) % taps, cb + (u + 1) / taps)
        }
    }
#undef F16A_STEP
#undef F16A_ISSUE

    // epilogue, wave-private (as conv_mfma_kernel's): every wave takes its (32 TM) x (32 TN) accumulators through a private f32 slab of
    // the two stages -- all fragment reads are behind the loop's closing barrier and no DMA is in flight -- from the C/D layout (column =
    // lane & 31 the output channel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) the pixel) to rows of 8 channels per lane: BN fold,
    // residual, ReLU in f32, one rounding to f16, one 16-byte store.  LDS operations of one wave execute in order: no barrier.
    {
        constexpr int WROWS = TM * 32, WCOLS = TN * 32;
        constexpr int L8 = WCOLS / 8;                        // lanes per row
        constexpr int RPW = 64 / L8;                         // rows per store iteration
        constexpr int NIT = WROWS / RPW;
        constexpr int PW = WROWS * WCOLS;
        static_assert(PW * 4 * 4 <= STAGE, "four wave-private slabs per stage");
        float *Ws = reinterpret_cast<float *>(wave < 4 ? stage0 : stage1) + (wave & 3) * PW;
        const int oct = lane % L8, rsub = lane / L8;
        const int co = n0 + wn * (BN / WN) + oct * 8;
        float sc[8], sh[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { sc[q] = a.scale ? a.scale[co + q] : 1.f; sh[q] = a.shift[co + q]; }      // fmaf(v, 1, shift) = v + shift bit for bit
        const int mw = m0 + wm * (BM / WM);                  // first output pixel of the wave's block
        // the residual rows are requested first, before the accumulators go through LDS
        f16x8 rvs[NIT];
        if (a.resid) {
#pragma unroll
            for (int it = 0; it < NIT; it++) {
                const int m = mw + it * RPW + rsub;
                f16x8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
                if (m < M) rv = *reinterpret_cast<const f16x8 *>(a.resid + (size_t)m * a.Cout + co);
                rvs[it] = rv;
            }
        }
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
                for (int jn = 0; jn < TN; jn++) Ws[row * WCOLS + jn * 32 + (lane & 31)] = acc[i][jn][r];
            }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int row = it * RPW + rsub;
            const int m = mw + row;
            const float4 v0 = *reinterpret_cast<const float4 *>(Ws + row * WCOLS + oct * 8);
            const float4 v1 = *reinterpret_cast<const float4 *>(Ws + row * WCOLS + oct * 8 + 4);
            float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            f16x8 o;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                float e = fmaf(v[q], sc[q], sh[q]);
                if (a.resid) e = e + (float)rvs[it][q];
                if (a.relu_out) e = fmaxf(e, 0.f);
                o[q] = f16_sat(e);
            }
            if (m < M) *reinterpret_cast<f16x8 *>(a.out + (size_t)m * a.Cout + co) = o;
        }
    }
}

template <int BM, int BN, int WM, int WN, int KS>
void launch_inst(const ConvF16Args &a, int M, int Ho, int Wo, hipStream_t s)
{
    const int nMt = (M + BM - 1) / BM, nNt = a.Cout / BN;
    const dim3 grid(((nMt + 7) / 8) * 8 * nNt);
    hipLaunchKernelGGL((conv_f16act_kernel<BM, BN, WM, WN, KS>), grid, dim3(512), 0, s, a, M, Ho, Wo, nMt, nNt, make_fdiv(Ho * Wo), make_fdiv(Wo));
}

}  // namespace

// Tile shapes as PREC = 3: 128 x 128; Cout = 64 (mod 128): 128 x 64 for 1 x 1, 256 x 64 for 3 x 3
bool launch_conv_f16act(const ConvF16Args &a, hipStream_t s)
{
    const int Ho = a.stride ? a.h / a.stride : 0, Wo = a.stride ? a.w / a.stride : 0;
    const long long Mll = (long long)a.N * Ho * Wo;
    const long long taps = (long long)a.ksize * a.ksize;
    if (!((a.ksize == 3 && a.stride == 1) || (a.ksize == 1 && (a.stride == 1 || a.stride == 2))) || a.Cin < 64 || a.Cin % 64 || a.Cout < 64 || a.Cout % 64 ||
        Mll <= 0 || Mll > 0x7fffffffLL / 2 || (long long)a.N * a.h * a.w > 0x7fffffffLL || Wo < 2 || a.h % a.stride || a.w % a.stride || !a.in || !a.W || !a.shift || !a.out ||
        taps * a.Cin * a.Cout * 2 > 0x7fffffffLL ||                                          // the weights behind one descriptor
        ((long long)4 * 256 + 2 * a.w + 4) * a.Cin * 2 > 0x7fffffffLL) {                     // a tile's stored pixels behind one descriptor
        set_error("launch_conv_f16act: unsupported shape");
        return false;
    }
    const int M = (int)Mll;
    if (a.Cout % 128 == 0) {
        if (a.ksize == 3) launch_inst<128, 128, 4, 2, 3>(a, M, Ho, Wo, s);
        else launch_inst<128, 128, 4, 2, 1>(a, M, Ho, Wo, s);
    } else if (a.ksize == 3) launch_inst<256, 64, 8, 1, 3>(a, M, Ho, Wo, s);
    else launch_inst<128, 64, 4, 2, 1>(a, M, Ho, Wo, s);
    return true;
}

}  // namespace tmat
