// PNG encoder: every rule of the byte stream, shared by png_host.cpp (host twin) and png_kernels.hip (device), which
// must produce the same file.  A file is a function of the picture and (H, W, channels) alone:
//   filter    one type per row out of None / Sub / Up / Average / Paeth: the minimum sum of |signed residual|, ties to the lowest number
//   stripes   the filtered stream (H rows of 1 + W channels bytes) is cut every PNG_STRIPE bytes; a stripe is compressed on its own,
//             matches never reach before its first byte, and it becomes one IDAT chunk
//   matches   per position the longest of four candidates -- distance 1, distance `channels`, distance of one row, and the position a
//             hash table of 3-byte strings returns -- capped at 258 and at the stripe's end; equal lengths keep the earlier candidate.
//             The table is read for a whole sub-chunk of PNG_SUB positions before any of them enters it, and an entry keeps the
//             HIGHEST position: both are independent of the order in which lanes arrive
//   parse     greedy from position 0: a match of 3 or more is taken, anything else is a literal
//   blocks    one fixed-Huffman block (BTYPE 01) or one stored block per stripe, whichever is fewer bytes (stored on a tie).  A
//             fixed block of a stripe that is not the last is closed at a byte boundary with an empty stored block; the last block
//             carries BFINAL.  The zlib header rides in the first stripe's chunk, the Adler-32 in a 4-byte IDAT chunk of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

namespace tmat {

constexpr int PNG_STRIPE = 8192;            // S: bytes of filtered stream per stripe (tmat_png_stripe)
constexpr int PNG_SUB = 256;                // sub-chunk of the hash-table walk = threads of the stripe workgroup
constexpr int PNG_HASH_BITS = 12;
constexpr int PNG_MAX_MATCH = 258, PNG_MIN_MATCH = 3;
constexpr int PNG_SLOT = PNG_STRIPE + 32;   // worst-case chunk of one stripe: 12 (chunk) + 2 (zlib header) + 5 (stored header) + S, rounded up
constexpr int PNG_HEAD = 33;                // signature + IHDR chunk
constexpr int PNG_TAIL = 28;                // Adler-32 IDAT chunk (16) + IEND chunk (12)
constexpr uint32_t PNG_ADLER_MOD = 65521;

struct PngShape {
    int H, W, ch;
    int rb;             // bytes of one raw row
    size_t raw;         // bytes of the filtered stream
    int ns;             // stripes
    size_t bound;       // worst-case file
};
// false for H, W < 1, channels outside {1, 3} or a filtered stream of 2^31 bytes or more
inline bool png_shape(int H, int W, int ch, PngShape &g)
{
    if (H < 1 || W < 1 || (ch != 1 && ch != 3)) return false;
    const unsigned long long rb = (unsigned long long)W * ch, raw = (unsigned long long)H * (rb + 1);
    if (raw >= (1ull << 31)) return false;
    g.H = H; g.W = W; g.ch = ch; g.rb = (int)rb; g.raw = (size_t)raw;
    g.ns = (int)((raw + PNG_STRIPE - 1) / PNG_STRIPE);
    g.bound = PNG_HEAD + (size_t)raw + (size_t)g.ns * 19 + PNG_TAIL;
    return true;
}

PNG_HD int png_paeth(int a, int b, int c)
{
    int p = a + b - c;
    int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// residual of filter type f for the byte x with left a, above b, above-left c
PNG_HD uint8_t png_residual(int f, int x, int a, int b, int c)
{
    int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
    return (uint8_t)(x - pred);
}
PNG_HD uint32_t png_absres(uint8_t r) { return r < 128 ? r : 256u - r; }

PNG_HD uint32_t png_hash3(const uint8_t *s)
{
    uint32_t v = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    return (v * 2654435761u) >> (32 - PNG_HASH_BITS);
}

// the match of position p in the stripe s[0, n): length | distance << 16, or 0.  cand1: 1 + the position the hash table gave, or 0
PNG_HD uint32_t png_best_match(const uint8_t *s, int n, int p, int cand1, int ch, int rowlen)
{
    const int maxl = n - p < PNG_MAX_MATCH ? n - p : PNG_MAX_MATCH;
    if (maxl < PNG_MIN_MATCH) return 0;
    int best = 0, bd = 0;
    for (int k = 0; k < 4; k++) {
        const int d = k == 0 ? 1 : k == 1 ? ch : k == 2 ? rowlen : (cand1 > 0 ? p - (cand1 - 1) : 0);
        if (d < 1 || d > p) continue;
        if (best >= maxl) break;
        if (s[p + best] != s[p + best - d]) continue;       // cannot be longer than the best so far
        int l = 0;
        while (l < maxl && s[p + l] == s[p + l - d]) l++;
        if (l > best) { best = l; bd = d; }
    }
    return best >= PNG_MIN_MATCH ? (uint32_t)best | ((uint32_t)bd << 16) : 0u;
}

PNG_HD uint32_t png_rev(uint32_t v, int bits)      // Huffman codes enter the stream from their most significant bit
{
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}
PNG_HD int png_log2(uint32_t v) { return 31 - __builtin_clz(v); }

// fixed-Huffman code of a literal / length symbol (0..287), as it enters the stream
PNG_HD uint32_t png_litlen_code(int sym, int &bits)
{
    if (sym < 144) { bits = 8; return png_rev(0x30 + sym, 8); }
    if (sym < 256) { bits = 9; return png_rev(0x190 + (sym - 144), 9); }
    if (sym < 280) { bits = 7; return png_rev(sym - 256, 7); }
    bits = 8;
    return png_rev(0xC0 + (sym - 280), 8);
}
// the bits of one token, at most 31: a literal (len 0, value lit) or a match (len 3..258, dist 1..32768)
PNG_HD uint32_t png_token(int len, int dist, int lit, int &bits)
{
    if (len == 0) return png_litlen_code(lit, bits);
    int lcode, lext, lval;
    const int l = len - 3;
    if (len == PNG_MAX_MATCH) { lcode = 28; lext = 0; lval = 0; }
    else if (l < 8) { lcode = l; lext = 0; lval = 0; }
    else { lext = png_log2((uint32_t)l) - 2; lcode = 4 * lext + 4 + ((l >> lext) & 3); lval = l & ((1 << lext) - 1); }
    int dcode, dext, dval;
    const int d = dist - 1;
    if (d < 4) { dcode = d; dext = 0; dval = 0; }
    else { dext = png_log2((uint32_t)d) - 1; dcode = 2 * dext + 2 + ((d >> dext) & 1); dval = d & ((1 << dext) - 1); }
    int nb;
    uint32_t v = png_litlen_code(257 + lcode, nb);
    v |= (uint32_t)lval << nb; nb += lext;
    v |= png_rev((uint32_t)dcode, 5) << nb; nb += 5;
    v |= (uint32_t)dval << nb; nb += dext;
    bits = nb;
    return v;
}

// bytes of the deflate data of a stripe of n bytes whose tokens take `tok_bits` bits, as a fixed block and as a stored block
PNG_HD uint32_t png_fixed_bytes(uint32_t tok_bits, bool last)
{
    const uint32_t t = 3 + tok_bits + 7;                 // block header, tokens, end of block
    return last ? (t + 7) / 8 : (t + 3 + 7) / 8 + 4;     // the joiner: a stored header, the pad, LEN = 0, NLEN = 0xffff
}
PNG_HD uint32_t png_stored_bytes(int n) { return 5u + (uint32_t)n; }

// CRC-32 (reflected, polynomial 0xedb88320).  png_crc_shift(c, k): the CRC of A || B from c = crc(A) and crc(B), for k = |B|, is
// png_crc_shift(c, k) ^ crc(B): products of polynomials modulo the CRC polynomial, x^(8k) by square and multiply.
PNG_HD uint32_t png_crc_byte(uint32_t c, uint8_t b)     // c: the running register (starts at ~0, complemented at the end)
{
    c ^= b;
    for (int i = 0; i < 8; i++) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
    return c;
}
PNG_HD uint32_t png_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
PNG_HD uint32_t png_crc_shift(uint32_t crc, uint32_t nbytes)
{
    uint32_t op = 0x80000000u, base = 0x00800000u;      // 1 and x^8
    for (uint32_t e = nbytes; e; e >>= 1) {
        if (e & 1u) op = png_gf_mul(op, base);
        base = png_gf_mul(base, base);
    }
    return png_gf_mul(op, crc);
}

// ---- host twin (png_host.cpp): one file into out[0, bound), *size its length; no GPU, no library ----
void png_encode_host(const uint8_t *pic, const PngShape &g, uint8_t *out, size_t *size);

#ifdef __HIPCC__
// ---- device (png_kernels.hip): k pictures of shape g at pics -> k files at files + i fcap, file_size[i] bytes each.
// filt: k g.raw bytes, slots: k g.ns PNG_SLOT bytes, meta: 4 k g.ns words, file_size: k words; fcap >= g.bound.  0 on success.
int png_encode_launch(const uint8_t *pics, int k, const PngShape &g, uint8_t *filt, uint8_t *slots, uint32_t *meta, uint8_t *files, size_t fcap,
                      uint32_t *file_size, hipStream_t s);
// n pictures (host or device memory) through the handle's stream and pool, in chunks that bound device memory: file i at
// out + i cap_each (host), sizes[i] its length; cap_each >= g.bound.  ms3 (nullable): += HIP-event ms of {upload, kernels, copy back}.
// Returns a TMAT_* code.  (tmat_api.cpp)
struct Ctx;
int png_encode_ctx(Ctx *c, const uint8_t *pics, bool on_host, int n, const PngShape &g, uint8_t *out, size_t cap_each, size_t *sizes, float *ms3);
#endif

}  // namespace tmat
