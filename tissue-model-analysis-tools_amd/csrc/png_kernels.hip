// PNG encoder on the device (the rules: png.h, the host twin: png_host.cpp).  Four launches per batch, no workgroup
// waits for another, every loop is bounded by the stripe length:
//   png_filter_kernel   one wave per row: the five residual sums, the choice, the filtered row
//   png_stripe_kernel   one workgroup per stripe: matches, greedy parse, bits packed in LDS, the chunk's CRC, Adler-32 partial sums;
//                       the finished IDAT chunk goes to the stripe's worst-case slot.  <true>: PNG_COMPACT (lazy parse, dynamic blocks)
//   png_layout_kernel   one workgroup per picture: prefix sum of the chunk sizes, Adler-32 combined, signature / IHDR / trailer written
//   png_gather_kernel   one workgroup per stripe: slot -> its place in the contiguous file
#include "png.h"
#include "dev_guard.h"

namespace tmat {

namespace {

constexpr int NT = PNG_SUB;                      // threads of the stripe workgroup
constexpr int SEG = PNG_STRIPE / NT;             // positions of the parse one thread owns
constexpr int OUT_WORDS = PNG_SLOT / 4;
static_assert(PNG_STRIPE % NT == 0 && NT == 256, "stripe geometry");
static_assert((1 << PNG_HASH_BITS) * 4 <= PNG_STRIPE * 2 && PNG_SLOT <= PNG_STRIPE * 2 && PNG_SLOT % 4 == 0, "the union buffer holds each of its three uses");
static_assert(PNG_STRIPE <= 32768, "distances and positions fit 16 bits");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    for (int o = 32; o; o >>= 1) v ^= __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t *__restrict__ pics, long long rows, int H, int rb, int bpp, uint8_t *__restrict__ filt)
{
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                       // whole waves leave; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int y = (int)(r % H);
    const uint8_t *cur = pics + (size_t)r * rb, *up = cur - rb;
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int x = lane; x < rb; x += 64) {
        const int a = x >= bpp ? cur[x - bpp] : 0, b = y ? up[x] : 0, c = (y && x >= bpp) ? up[x - bpp] : 0, v = cur[x];
#pragma unroll
        for (int f = 0; f < 5; f++) sum[f] += png_absres(png_residual(f, v, a, b, c));
    }
    int f = 0;
    uint32_t best = wave_sum(sum[0]);
#pragma unroll
    for (int k = 1; k < 5; k++) {
        const uint32_t t = wave_sum(sum[k]);
        if (t < best) { best = t; f = k; }
    }
    uint8_t *o = filt + (size_t)r * (rb + 1);
    if (lane == 0) o[0] = (uint8_t)f;
    for (int x = lane; x < rb; x += 64) {
        const int a = x >= bpp ? cur[x - bpp] : 0, b = y ? up[x] : 0, c = (y && x >= bpp) ? up[x - bpp] : 0;
        o[1 + x] = png_residual(f, cur[x], a, b, c);
    }
}

// bits [pos, pos + bits) of the zeroed word buffer w (cap_words words) |= v; false when they would leave the buffer
__device__ __forceinline__ bool put_bits(uint32_t *w, int cap_words, uint32_t pos, uint32_t v, int bits)
{
    if (bits == 0) return true;
    const uint32_t wi = pos >> 5, sh = pos & 31;
    if ((pos + bits + 31) / 32 > (uint32_t)cap_words) return false;
    atomicOr(&w[wi], v << sh);
    if (sh + bits > 32) atomicOr(&w[wi + 1], v >> (32 - sh));
    return true;
}

// meta per stripe: {chunk bytes, Adler sum of bytes mod 65521, Adler weighted sum mod 65521, offset in the file (png_layout_kernel)}
// COMPACT (PNG_COMPACT): the lazy parse, histograms by LDS atomics over the first walk, one lane builds the code lengths and tables with
// the host's own functions (png_dyn_plan, png_canonical; its scratch is the union region, free between the parse and the zeroing of the
// chunk), a second walk counts the dynamic block's bits per thread, the third emits.  A template parameter: the fast kernel holds none of it
template <bool COMPACT>
__global__ __launch_bounds__(NT) void png_stripe_kernel(const uint8_t *__restrict__ filt, size_t raw, int ns, int ch, int rowlen,
                                                         uint8_t *__restrict__ slots, uint32_t *__restrict__ meta)
{
    __shared__ uint8_t s_data[PNG_STRIPE];
    __shared__ uint32_t s_m[PNG_STRIPE];
    __shared__ uint32_t s_u[PNG_STRIPE / 2];     // in turn: the hash table, the parse's exit positions (u16), [compact: scratch], the chunk being built
    __shared__ uint16_t s_entry[NT];
    __shared__ uint32_t s_red[12];
    __shared__ int s_bad;
    __shared__ uint32_t s_ll[COMPACT ? PNG_NLL : 1], s_d[COMPACT ? PNG_ND : 1], s_cl[COMPACT ? PNG_NCL : 1];     // histograms, then code tables
    __shared__ PngDyn s_dyn;
    uint16_t *s_exit = (uint16_t *)s_u;
    uint8_t *s_out = (uint8_t *)s_u;
    static_assert(PNG_WS_WORDS <= PNG_STRIPE / 2, "the union buffer holds the scratch of the code lengths");

    const int t = threadIdx.x, k = blockIdx.x, pic = blockIdx.y, lane = t & 63, wv = t >> 6;
    const size_t b0 = (size_t)k * PNG_STRIPE;
    const int n = (int)(raw - b0 < (size_t)PNG_STRIPE ? raw - b0 : (size_t)PNG_STRIPE);      // 1 .. S: the grid has ceil(raw / S) stripes
    const bool last = k == ns - 1;
    const uint8_t *src = filt + (size_t)pic * raw + b0;

    for (int j = t; j < n; j += NT) s_data[j] = src[j];
    for (int j = t; j < (1 << PNG_HASH_BITS); j += NT) s_u[j] = 0;
    s_entry[t] = 0xffff;
    if (t == 0) s_bad = 0;
    if constexpr (COMPACT) {
        for (int j = t; j < PNG_NLL; j += NT) s_ll[j] = 0;
        if (t < PNG_ND) s_d[t] = 0;
    }
    __syncthreads();

    // Adler-32 partial sums over this thread's SEG bytes (at most 32 * 8192 * 255 per thread)
    uint32_t a1 = 0, a2 = 0;
    for (int j = t * SEG; j < min(n, (t + 1) * SEG); j++) { a1 += s_data[j]; a2 += (uint32_t)(n - j) * s_data[j]; }
    a2 %= PNG_ADLER_MOD;

    // matches: the table is read by the whole sub-chunk, then updated with the maximum -- independent of lane order
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int p = c0 + t;
        const bool in = p + 2 < n;
        const uint32_t h = in ? png_hash3(s_data + p) : 0;
        const int cand = in ? (int)s_u[h] : 0;
        __syncthreads();
        if (in) atomicMax(&s_u[h], (uint32_t)p + 1);
        if (p < n) s_m[p] = png_best_match(s_data, n, p, cand, ch, rowlen);
        __syncthreads();
    }

    // the parse (greedy, or lazy when compact): per thread the exit of every position of its segment, one lane hops over the segments,
    // then every segment is walked from its entry
    const int seg0 = t * SEG, seg1 = min(n, seg0 + SEG);
    for (int p = seg1 - 1; p >= seg0; p--) {
        const int len = png_take(s_m, n, p, COMPACT);
        const int nx = p + (len ? len : 1);
        s_exit[p] = (uint16_t)(nx >= seg1 ? nx : s_exit[nx]);
    }
    __syncthreads();
    if (t == 0) {
        int e = 0;
        for (int it = 0; it < NT && e < n; it++) { s_entry[e / SEG] = (uint16_t)e; e = s_exit[e]; }
    }
    __syncthreads();
    const int entry = s_entry[t];
    uint32_t my_bits = 0, my_extra = 0;
    if (entry != 0xffff)
        for (int p = entry; p < seg1;) {
            int bits;
            const uint32_t mm = s_m[p];
            const int len = png_take(s_m, n, p, COMPACT);
            png_token(len, (int)(mm >> 16), s_data[p], bits);
            my_bits += (uint32_t)bits;
            if constexpr (COMPACT) {
                if (len == 0) atomicAdd(&s_ll[s_data[p]], 1u);
                else {
                    int code, ext, val;
                    png_len_sym(len, code, ext, val);
                    atomicAdd(&s_ll[257 + code], 1u); my_extra += (uint32_t)ext;
                    png_dist_sym((int)(mm >> 16), code, ext, val);
                    atomicAdd(&s_d[code], 1u); my_extra += (uint32_t)ext;
                }
            }
            p += len ? len : 1;
        }
    // exclusive prefix sum of my_bits over the workgroup
    uint32_t incl = my_bits;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) s_red[wv] = incl;
    if constexpr (COMPACT) {
        my_extra = wave_sum(my_extra);
        if (lane == 0) s_red[4 + wv] = my_extra;
    } else {
        for (int j = t; j < OUT_WORDS; j += NT) s_u[j] = 0;      // the exits are dead: the region becomes the zeroed chunk
    }
    __syncthreads();
    uint32_t base_bits = 0, tok_bits = 0;
    for (int w = 0; w < 4; w++) { if (w < wv) base_bits += s_red[w]; tok_bits += s_red[w]; }
    uint32_t excl = base_bits + incl - my_bits;

    const int pre = k == 0 ? 2 : 0;
    const uint32_t fixed = png_fixed_bytes(tok_bits, last), stored = png_stored_bytes(n);
    int kind = fixed < stored ? 1 : 0;               // 0 stored, 1 fixed, 2 dynamic
    uint32_t bytes = kind ? fixed : stored;
    uint32_t dyn_tok = 0;                            // bits of the dynamic block's tokens
    if constexpr (COMPACT) {
        if (t == 0) {                                // the exits are dead: the region is this lane's scratch
            s_ll[256] += 1;
            png_dyn_plan(s_ll, s_d, s_red[4] + s_red[5] + s_red[6] + s_red[7], s_dyn, s_u);
            png_canonical(s_dyn.ll_len, PNG_NLL, s_ll, s_u);
            png_canonical(s_dyn.d_len, PNG_ND, s_d, s_u);
            png_canonical(s_dyn.cl_len, PNG_NCL, s_cl, s_u);
        }
        __syncthreads();
        const uint32_t dyn = png_block_bytes(s_dyn.bits, last);
        if (dyn < bytes) { kind = 2; bytes = dyn; }
        for (int j = t; j < OUT_WORDS; j += NT) s_u[j] = 0;      // the scratch is dead: the region becomes the zeroed chunk
        if (kind == 2) {                             // the whole workgroup or none of it: the choice is made from shared values
            my_bits = 0;
            if (entry != 0xffff)
                for (int p = entry; p < seg1;) {
                    uint32_t v1, v2;
                    int b1, b2;
                    const int len = png_take(s_m, n, p, true);
                    png_dyn_token(s_ll, s_d, len, (int)(s_m[p] >> 16), s_data[p], v1, b1, v2, b2);
                    my_bits += (uint32_t)(b1 + b2);
                    p += len ? len : 1;
                }
            incl = my_bits;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
            if (lane == 63) s_red[wv] = incl;        // every thread has read the fixed block's sums before the barrier above
        }
        __syncthreads();
        if (kind == 2) {
            base_bits = 0;
            for (int w = 0; w < 4; w++) { if (w < wv) base_bits += s_red[w]; dyn_tok += s_red[w]; }
            excl = base_bits + incl - my_bits;
        }
    }
    const bool use_block = kind != 0 && 12u + pre + bytes <= (uint32_t)PNG_SLOT;
    if (use_block) {
        uint32_t pos = (8 + pre) * 8 + (COMPACT && kind == 2 ? s_dyn.hdr : 3u) + excl;
        bool ok = true;
        if (entry != 0xffff)
            for (int p = entry; p < seg1;) {
                const uint32_t mm = s_m[p];
                const int len = png_take(s_m, n, p, COMPACT);
                if (!COMPACT || kind == 1) {
                    int bits;
                    const uint32_t v = png_token(len, (int)(mm >> 16), s_data[p], bits);
                    ok = put_bits(s_u, OUT_WORDS, pos, v, bits) && ok;
                    pos += bits;
                } else {                             // up to 48 bits: the literal or length, then the distance
                    uint32_t v1, v2;
                    int b1, b2;
                    png_dyn_token(s_ll, s_d, len, (int)(mm >> 16), s_data[p], v1, b1, v2, b2);
                    ok = put_bits(s_u, OUT_WORDS, pos, v1, b1) && ok;
                    ok = put_bits(s_u, OUT_WORDS, pos + b1, v2, b2) && ok;
                    pos += b1 + b2;
                }
                p += len ? len : 1;
            }
        if (t == 0) {
            if (!COMPACT || kind == 1) ok = put_bits(s_u, OUT_WORDS, (8 + pre) * 8, (last ? 1u : 0u) | 2u, 3) && ok;
            else {
                uint32_t hp = (8 + pre) * 8;
                png_dyn_header(s_dyn, s_cl, last, [&](uint32_t v, int bits) { ok = put_bits(s_u, OUT_WORDS, hp, v, bits) && ok; hp += bits; });
                ok = put_bits(s_u, OUT_WORDS, (8 + pre) * 8 + s_dyn.hdr + dyn_tok, s_ll[256] & 0xffffu, (int)(s_ll[256] >> 16)) && ok;
            }
            if (!last) ok = put_bits(s_u, OUT_WORDS, (8 + pre + bytes - 4) * 8, 0xffff0000u, 32) && ok;
        }
        if (!ok) s_bad = 1;
    }
    __syncthreads();
    const bool block_done = use_block && !s_bad;     // a write refused by the capacity check: the stripe is stored instead
    __syncthreads();
    if (!block_done) {
        if (use_block) {                             // clear what the refused attempt left
            for (int j = t; j < OUT_WORDS; j += NT) s_u[j] = 0;
            __syncthreads();
        }
        uint8_t *d = s_out + 8 + pre;
        if (t == 0) {
            d[0] = last ? 1 : 0;
            d[1] = (uint8_t)n; d[2] = (uint8_t)(n >> 8);
            d[3] = (uint8_t)~n; d[4] = (uint8_t)(~n >> 8);
        }
        for (int j = t; j < n; j += NT) d[5 + j] = s_data[j];
    }
    const uint32_t dlen = pre + (block_done ? bytes : stored);
    if (t == 0) {
        s_out[0] = (uint8_t)(dlen >> 24); s_out[1] = (uint8_t)(dlen >> 16); s_out[2] = (uint8_t)(dlen >> 8); s_out[3] = (uint8_t)dlen;
        s_out[4] = 'I'; s_out[5] = 'D'; s_out[6] = 'A'; s_out[7] = 'T';
        if (pre) { s_out[8] = 0x78; s_out[9] = 0x01; }
    }
    __syncthreads();

    // CRC-32 of type + data: every thread its piece, moved to the end of the message, all pieces xor-ed
    const uint32_t clen = 4 + dlen, piece = (clen + NT - 1) / NT;
    const uint32_t c0 = min(clen, (uint32_t)t * piece), c1 = min(clen, c0 + piece);
    uint32_t crc = 0;
    if (c1 > c0) {
        uint32_t c = 0xffffffffu;
        for (uint32_t j = c0; j < c1; j++) c = png_crc_byte(c, s_out[4 + j]);
        crc = png_crc_shift(~c, clen - c1);
    }
    crc = wave_xor(crc);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) { s_red[wv] = crc; s_red[4 + wv] = a1; s_red[8 + wv] = a2; }
    __syncthreads();
    const uint32_t total = 12 + dlen;                // <= PNG_SLOT by the choice above
    if (t == 0) {
        const uint32_t v = s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3];
        uint8_t *q = s_out + 8 + dlen;
        q[0] = (uint8_t)(v >> 24); q[1] = (uint8_t)(v >> 16); q[2] = (uint8_t)(v >> 8); q[3] = (uint8_t)v;
        uint32_t *mt = meta + 4 * ((size_t)pic * ns + k);
        mt[0] = total;
        mt[1] = (s_red[4] + s_red[5] + s_red[6] + s_red[7]) % PNG_ADLER_MOD;
        mt[2] = (s_red[8] + s_red[9] + s_red[10] + s_red[11]) % PNG_ADLER_MOD;
    }
    __syncthreads();
    uint32_t *dst = (uint32_t *)(slots + ((size_t)pic * ns + k) * PNG_SLOT);       // slots are 4-byte aligned: PNG_SLOT % 4 == 0
    for (uint32_t j = t; j < (total + 3) / 4 && j < (uint32_t)OUT_WORDS; j += NT) dst[j] = s_u[j];
}

__device__ __forceinline__ void put_be32_dev(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
// length and CRC around the n data bytes at p + 8 of a chunk whose type is at p + 4 (one thread: header and trailer chunks only)
__device__ void close_chunk_dev(uint8_t *p, uint32_t n)
{
    put_be32_dev(p, n);
    uint32_t c = 0xffffffffu;
    for (uint32_t j = 0; j < 4 + n; j++) c = png_crc_byte(c, p[4 + j]);
    put_be32_dev(p + 8 + n, ~c);
}

__global__ __launch_bounds__(256) void png_layout_kernel(uint32_t *__restrict__ meta, int ns, size_t raw, int H, int W, int ch, uint8_t *__restrict__ files,
                                                          size_t fcap, uint32_t *__restrict__ file_size)
{
    __shared__ uint32_t s_sum[4], s_a[4], s_b[4];
    const int t = threadIdx.x, pic = blockIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t *mt = meta + 4 * (size_t)pic * ns;
    const int per = (ns + 255) / 256, k0 = min(ns, t * per), k1 = min(ns, k0 + per);
    uint32_t bytes = 0;
    unsigned long long a = 0, b = 0;
    for (int k = k0; k < k1; k++) {
        bytes += mt[4 * k];
        const size_t end = min(raw, ((size_t)k + 1) * PNG_STRIPE);
        const unsigned long long after = (raw - end) % PNG_ADLER_MOD;
        a += mt[4 * k + 1];
        b = (b + mt[4 * k + 2] + (unsigned long long)mt[4 * k + 1] * after) % PNG_ADLER_MOD;
    }
    uint32_t incl = bytes;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    const uint32_t wa = wave_sum((uint32_t)(a % PNG_ADLER_MOD)), wb = wave_sum((uint32_t)b);
    if (lane == 63) s_sum[wv] = incl;
    if (lane == 0) { s_a[wv] = wa; s_b[wv] = wb; }
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int w = 0; w < 4; w++) { if (w < wv) base += s_sum[w]; all += s_sum[w]; }
    uint32_t off = PNG_HEAD + base + incl - bytes;
    for (int k = k0; k < k1; k++) { mt[4 * k + 3] = off; off += mt[4 * k]; }
    if (t == 0) {
        const size_t size = (size_t)PNG_HEAD + all + PNG_TAIL;
        if (size > fcap) { file_size[pic] = 0; return; }         // cannot happen for fcap >= the bound; never write past the file's room
        uint8_t *f = files + (size_t)pic * fcap;
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        for (int j = 0; j < 8; j++) f[j] = sig[j];
        uint8_t *c = f + 8;
        c[4] = 'I'; c[5] = 'H'; c[6] = 'D'; c[7] = 'R';
        put_be32_dev(c + 8, (uint32_t)W);
        put_be32_dev(c + 12, (uint32_t)H);
        c[16] = 8; c[17] = ch == 1 ? 0 : 2; c[18] = 0; c[19] = 0; c[20] = 0;
        close_chunk_dev(c, 13);
        const uint32_t A = (1 + s_a[0] + s_a[1] + s_a[2] + s_a[3]) % PNG_ADLER_MOD;
        const uint32_t B = (uint32_t)((raw % PNG_ADLER_MOD + s_b[0] + s_b[1] + s_b[2] + s_b[3]) % PNG_ADLER_MOD);
        c = f + PNG_HEAD + all;
        c[4] = 'I'; c[5] = 'D'; c[6] = 'A'; c[7] = 'T';
        put_be32_dev(c + 8, (B << 16) | A);
        close_chunk_dev(c, 4);
        c += 16;
        c[4] = 'I'; c[5] = 'E'; c[6] = 'N'; c[7] = 'D';
        close_chunk_dev(c, 0);
        file_size[pic] = (uint32_t)size;
    }
}

__global__ __launch_bounds__(256) void png_gather_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ meta, int ns, uint8_t *__restrict__ files,
                                                          size_t fcap)
{
    const int k = blockIdx.x, pic = blockIdx.y;
    const uint32_t *mt = meta + 4 * ((size_t)pic * ns + k);
    const uint32_t bytes = mt[0], off = mt[3];
    if (bytes > (uint32_t)PNG_SLOT || (size_t)off + bytes + PNG_TAIL > fcap) return;      // never past the slot or the file's room
    const uint8_t *src = slots + ((size_t)pic * ns + k) * PNG_SLOT;
    uint8_t *dst = files + (size_t)pic * fcap + off;
    for (uint32_t j = threadIdx.x; j < bytes; j += 256) dst[j] = src[j];
}

// tmat_debug_png_code_lengths: histogram i of n symbols -> its code lengths, one lane each (the scratch is private memory here)
__global__ __launch_bounds__(64) void png_code_lengths_kernel(const uint32_t *__restrict__ freqs, int k, int n, int limit, uint8_t *__restrict__ lens)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < k) png_code_lengths(freqs + (size_t)i * n, n, limit, lens + (size_t)i * n);
}

}  // namespace

int png_code_lengths_launch(const uint32_t *freqs, int k, int n, int limit, uint8_t *lens, hipStream_t s)
{
    if (k < 1 || n < 1 || n > PNG_NLL || limit < 1 || limit > 15 || (1 << limit) < n) return -1;
    hipLaunchKernelGGL(png_code_lengths_kernel, dim3((k + 63) / 64), dim3(64), 0, s, freqs, k, n, limit, lens);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int png_encode_launch(const uint8_t *pics, int k, const PngShape &g, int mode, uint8_t *filt, uint8_t *slots, uint32_t *meta, uint8_t *files, size_t fcap,
                      uint32_t *file_size, hipStream_t s)
{
    if (k < 1 || k > 65535 || fcap < g.bound || (mode != PNG_FAST && mode != PNG_COMPACT)) return -1;
    const long long rows = (long long)k * g.H;
    if ((rows + 3) / 4 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, pics, rows, g.H, g.rb, g.ch, filt);
    if (mode == PNG_COMPACT)
        hipLaunchKernelGGL(png_stripe_kernel<true>, dim3(g.ns, k), dim3(NT), 0, s, (const uint8_t *)filt, g.raw, g.ns, g.ch, g.rb + 1, slots, meta);
    else
        hipLaunchKernelGGL(png_stripe_kernel<false>, dim3(g.ns, k), dim3(NT), 0, s, (const uint8_t *)filt, g.raw, g.ns, g.ch, g.rb + 1, slots, meta);
    hipLaunchKernelGGL(png_layout_kernel, dim3(k), dim3(256), 0, s, meta, g.ns, g.raw, g.H, g.W, g.ch, files, fcap, file_size);
    hipLaunchKernelGGL(png_gather_kernel, dim3(g.ns, k), dim3(256), 0, s, (const uint8_t *)slots, (const uint32_t *)meta, g.ns, files, fcap);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace tmat
