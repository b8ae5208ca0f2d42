// Host twin of the PNG encoder (png_kernels.hip): the rules of png.h applied one byte after the other.  Same bytes as the device,
// no GPU, no compression library.
#include "png.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace tmat {

namespace {

struct Crc {
    uint32_t c = 0xffffffffu;
    void add(const uint8_t *p, size_t n) { for (size_t i = 0; i < n; i++) c = png_crc_byte(c, p[i]); }
    uint32_t value() const { return ~c; }
};

void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// chunk `type` with n data bytes already at p + 8: length in front, CRC behind; returns the chunk's size
size_t close_chunk(uint8_t *p, const char *type, size_t n)
{
    put_be32(p, (uint32_t)n);
    std::memcpy(p + 4, type, 4);
    Crc crc;
    crc.add(p + 4, 4 + n);
    put_be32(p + 8 + n, crc.value());
    return 12 + n;
}

void filter_rows(const uint8_t *pic, const PngShape &g, uint8_t *filt)
{
    const int rb = g.rb, bpp = g.ch;
    for (int y = 0; y < g.H; y++) {
        const uint8_t *cur = pic + (size_t)y * rb, *up = y ? cur - rb : nullptr;
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (int x = 0; x < rb; x++) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            for (int f = 0; f < 5; f++) sum[f] += png_absres(png_residual(f, cur[x], a, b, c));
        }
        int f = 0;
        for (int k = 1; k < 5; k++) if (sum[k] < sum[f]) f = k;
        uint8_t *o = filt + (size_t)y * (rb + 1);
        o[0] = (uint8_t)f;
        for (int x = 0; x < rb; x++) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            o[1 + x] = png_residual(f, cur[x], a, b, c);
        }
    }
}

struct BitWriter {
    uint8_t *p;
    size_t cap, bit = 0;
    bool ok = true;
    BitWriter(uint8_t *dst, size_t capacity) : p(dst), cap(capacity) { std::memset(p, 0, cap); }
    void put(uint32_t v, int bits)
    {
        if (bit + bits > cap * 8) { ok = false; return; }       // never past the slot
        for (int i = 0; i < bits; i++, bit++) p[bit >> 3] |= (uint8_t)(((v >> i) & 1u) << (bit & 7));
    }
    void align() { bit = (bit + 7) & ~(size_t)7; }
};

// the deflate data of the stripe s[0, n) into dst[0, cap) in the given mode; returns its length
size_t deflate_stripe(const uint8_t *s, int n, bool last, int ch, int rowlen, int mode, uint8_t *dst, size_t cap, std::vector<uint32_t> &m)
{
    std::vector<uint32_t> table((size_t)1 << PNG_HASH_BITS, 0);
    int cand[PNG_SUB];
    for (int c0 = 0; c0 < n; c0 += PNG_SUB) {
        const int e = std::min(n, c0 + PNG_SUB);
        for (int p = c0; p < e; p++) cand[p - c0] = p + 2 < n ? (int)table[png_hash3(s + p)] : 0;
        for (int p = c0; p < e; p++)
            if (p + 2 < n) { uint32_t &t = table[png_hash3(s + p)]; t = std::max(t, (uint32_t)p + 1); }
        for (int p = c0; p < e; p++) m[p] = png_best_match(s, n, p, cand[p - c0], ch, rowlen);
    }
    const bool compact = mode == PNG_COMPACT;
    uint32_t tok_bits = 0, extra_bits = 0, llf[PNG_NLL] = {0}, df[PNG_ND] = {0};
    for (int p = 0; p < n;) {
        int bits;
        const int len = png_take(m.data(), n, p, compact), dist = (int)(m[p] >> 16);
        png_token(len, dist, s[p], bits);
        tok_bits += (uint32_t)bits;
        if (compact) {
            if (len == 0) llf[s[p]]++;
            else {
                int code, ext, val;
                png_len_sym(len, code, ext, val);
                llf[257 + code]++; extra_bits += (uint32_t)ext;
                png_dist_sym(dist, code, ext, val);
                df[code]++; extra_bits += (uint32_t)ext;
            }
        }
        p += len ? len : 1;
    }
    const uint32_t fixed = png_fixed_bytes(tok_bits, last), stored = png_stored_bytes(n);
    int kind = fixed < stored ? 1 : 0;              // 0 stored, 1 fixed, 2 dynamic
    uint32_t bytes = kind ? fixed : stored;
    PngDyn D;
    uint32_t ws[PNG_WS_WORDS], llc[PNG_NLL], dc[PNG_ND], clc[PNG_NCL];
    if (compact) {
        llf[256]++;
        png_dyn_plan(llf, df, extra_bits, D, ws);
        const uint32_t dyn = png_block_bytes(D.bits, last);
        if (dyn < bytes) { kind = 2; bytes = dyn; }
    }
    if (kind && bytes <= cap) {
        BitWriter w(dst, bytes);
        if (kind == 1) w.put((last ? 1u : 0u) | 2u, 3);
        else {
            png_canonical(D.ll_len, PNG_NLL, llc, ws);
            png_canonical(D.d_len, PNG_ND, dc, ws);
            png_canonical(D.cl_len, PNG_NCL, clc, ws);
            png_dyn_header(D, clc, last, [&](uint32_t v, int bits) { w.put(v, bits); });
        }
        for (int p = 0; p < n;) {
            const int len = png_take(m.data(), n, p, compact), dist = (int)(m[p] >> 16);
            if (kind == 1) {
                int bits;
                const uint32_t v = png_token(len, dist, s[p], bits);
                w.put(v, bits);
            } else {
                uint32_t v1, v2;
                int b1, b2;
                png_dyn_token(llc, dc, len, dist, s[p], v1, b1, v2, b2);
                w.put(v1, b1);
                w.put(v2, b2);
            }
            p += len ? len : 1;
        }
        if (kind == 1) w.put(0, 7); else w.put(llc[256] & 0xffffu, (int)(llc[256] >> 16));
        if (!last) { w.put(0, 3); w.align(); w.put(0xffff0000u, 32); }
        if (w.ok) return bytes;
    }
    dst[0] = last ? 1 : 0;
    dst[1] = (uint8_t)n; dst[2] = (uint8_t)(n >> 8);
    dst[3] = (uint8_t)~n; dst[4] = (uint8_t)(~n >> 8);
    std::memcpy(dst + 5, s, (size_t)n);
    return stored;
}

}  // namespace

void png_encode_host(const uint8_t *pic, const PngShape &g, int mode, uint8_t *out, size_t *size)
{
    std::vector<uint8_t> filt(g.raw);
    filter_rows(pic, g, filt.data());
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    uint8_t *o = out;
    std::memcpy(o, sig, 8);
    o += 8;
    put_be32(o + 8, (uint32_t)g.W);
    put_be32(o + 12, (uint32_t)g.H);
    o[16] = 8; o[17] = g.ch == 1 ? 0 : 2; o[18] = 0; o[19] = 0; o[20] = 0;
    o += close_chunk(o, "IHDR", 13);
    std::vector<uint32_t> m(PNG_STRIPE);
    uint8_t slot[PNG_SLOT];
    uint64_t s1 = 0, s2 = 0;        // Adler-32: 1 + sum of bytes, and the sum of those running sums
    for (int k = 0; k < g.ns; k++) {
        const size_t b0 = (size_t)k * PNG_STRIPE;
        const int n = (int)std::min<size_t>(PNG_STRIPE, g.raw - b0);
        const uint8_t *s = filt.data() + b0;
        const int pre = k == 0 ? 2 : 0;
        if (pre) { slot[8] = 0x78; slot[9] = 0x01; }
        const size_t dl = deflate_stripe(s, n, k == g.ns - 1, g.ch, g.rb + 1, mode, slot + 8 + pre, PNG_SLOT - 12 - pre, m);
        const size_t total = close_chunk(slot, "IDAT", pre + dl);
        std::memcpy(o, slot, total);
        o += total;
        uint64_t a = 0, b = 0;
        for (int j = 0; j < n; j++) { a += s[j]; b += (uint64_t)(n - j) * s[j]; }
        const uint64_t after = (g.raw - b0 - n) % PNG_ADLER_MOD;
        s1 = (s1 + a) % PNG_ADLER_MOD;
        s2 = (s2 + b % PNG_ADLER_MOD + (a % PNG_ADLER_MOD) * after) % PNG_ADLER_MOD;
    }
    const uint32_t A = (uint32_t)((1 + s1) % PNG_ADLER_MOD), B = (uint32_t)((g.raw % PNG_ADLER_MOD + s2) % PNG_ADLER_MOD);
    put_be32(o + 8, (B << 16) | A);
    o += close_chunk(o, "IDAT", 4);
    o += close_chunk(o, "IEND", 0);
    *size = (size_t)(o - out);
}

}  // namespace tmat
