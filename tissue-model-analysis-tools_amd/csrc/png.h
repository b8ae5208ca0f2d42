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
// The above is the mode PNG_FAST.  PNG_COMPACT (opt-in) keeps filter, stripes and matches and changes two rules:
//   parse     one-step lazy (png_take): a match at p gives way to a literal when the match at p + 1 is longer; the rule applies again there
//   blocks    stored, fixed or dynamic Huffman (BTYPE 10) per stripe, by exact byte counts known before a bit is written: the fewest
//             bytes win, the earlier of the three on a tie.  The dynamic block's code lengths come from png_code_lengths over the
//             stripe's histograms (png_dyn_plan), its header is trimmed and run-length coded by png_rle_step, its codes are canonical
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
constexpr int PNG_FAST = 0, PNG_COMPACT = 1;                    // TMAT_PNG_FAST, TMAT_PNG_COMPACT
constexpr int PNG_NLL = 286, PNG_ND = 30, PNG_NCL = 19;         // alphabets: literal / length, distance, code length
constexpr int PNG_WS_WORDS = 2 * PNG_NLL + 128 + PNG_NCL + 13;  // scratch words of png_code_lengths_ws (2 n + 128) with png_dyn_plan's histogram behind

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
// length 3..258 -> its symbol 257 + code, the count and the value of its extra bits; the same for a distance 1..32768 (symbol = code)
PNG_HD void png_len_sym(int len, int &code, int &ext, int &val)
{
    const int l = len - 3;
    if (len == PNG_MAX_MATCH) { code = 28; ext = 0; val = 0; }
    else if (l < 8) { code = l; ext = 0; val = 0; }
    else { ext = png_log2((uint32_t)l) - 2; code = 4 * ext + 4 + ((l >> ext) & 3); val = l & ((1 << ext) - 1); }
}
PNG_HD void png_dist_sym(int dist, int &code, int &ext, int &val)
{
    const int d = dist - 1;
    if (d < 4) { code = d; ext = 0; val = 0; }
    else { ext = png_log2((uint32_t)d) - 1; code = 2 * ext + 2 + ((d >> ext) & 1); val = d & ((1 << ext) - 1); }
}
// the bits of one token in a fixed block, at most 31: a literal (len 0, value lit) or a match (len 3..258, dist 1..32768)
PNG_HD uint32_t png_token(int len, int dist, int lit, int &bits)
{
    if (len == 0) return png_litlen_code(lit, bits);
    int lcode, lext, lval, dcode, dext, dval;
    png_len_sym(len, lcode, lext, lval);
    png_dist_sym(dist, dcode, dext, dval);
    int nb;
    uint32_t v = png_litlen_code(257 + lcode, nb);
    v |= (uint32_t)lval << nb; nb += lext;
    v |= png_rev((uint32_t)dcode, 5) << nb; nb += 5;
    v |= (uint32_t)dval << nb; nb += dext;
    bits = nb;
    return v;
}

// the parse: the length of the match taken at p (0: a literal) from the matches m[0, n) of the stripe.  lazy (PNG_COMPACT): a match
// gives way when the next position's is longer.  The successor p + max(1, png_take) is a function of p alone in both modes
PNG_HD int png_take(const uint32_t *m, int n, int p, bool lazy)
{
    int len = (int)(m[p] & 0xffff);
    if (lazy && len && p + 1 < n && (int)(m[p + 1] & 0xffff) > len) len = 0;
    return len;
}

// bytes of the deflate data of a stripe of n bytes whose tokens take `tok_bits` bits, as a fixed block and as a stored block
PNG_HD uint32_t png_fixed_bytes(uint32_t tok_bits, bool last)
{
    const uint32_t t = 3 + tok_bits + 7;                 // block header, tokens, end of block
    return last ? (t + 7) / 8 : (t + 3 + 7) / 8 + 4;     // the joiner: a stored header, the pad, LEN = 0, NLEN = 0xffff
}
PNG_HD uint32_t png_stored_bytes(int n) { return 5u + (uint32_t)n; }
// the same for any coded block of t bits, its 3 header bits and its end of block included
PNG_HD uint32_t png_block_bytes(uint32_t t, bool last) { return last ? (t + 7) / 8 : (t + 3 + 7) / 8 + 4; }

// ---- PNG_COMPACT: dynamic Huffman blocks (RFC 1951 3.2.7) ----

// Code lengths of the histogram freq[0, n): len[i] = 0 exactly where freq[i] = 0, none above limit, Kraft sum exactly 1 -- but a lone
// used symbol gets the one-bit code (no complete set has one member; the callers below never ask for it).  n <= PNG_NLL, 2^limit >= n,
// limit <= 15, the sum of the frequencies below 2^22; ws: 2 n + 128 words.  Deterministic, every loop bounded by n, 128 or limit:
//   order     used symbols by (frequency, index): a stable radix sort, 7 bits a pass
//   tree      Huffman by Moffat and Katajainen's in-place two-queue merge (a tie between a leaf and a tree takes the leaf, which keeps
//             the tree shallow); optimal, so where no length exceeds the limit the total cost is the optimum
//   limit     longer codes are cut to the limit; while the set is over-subscribed, one code of the limit is dropped together with one of
//             the longest shorter length b, for two of b + 1 (each step lowers the Kraft sum by 2^-limit); at most one step per symbol
//   assign    the counts per length go to the symbols in sorted order, the longest to the least frequent
PNG_HD void png_code_lengths_ws(const uint32_t *freq, int n, int limit, uint8_t *len, uint32_t *ws)
{
    uint32_t *ka = ws, *kb = ws + n, *cnt = ws + 2 * n;
    int m = 0;
    uint32_t maxf = 0;
    for (int i = 0; i < n; i++) {
        len[i] = 0;
        if (freq[i]) { ka[m++] = (freq[i] << 9) | (uint32_t)i; if (freq[i] > maxf) maxf = freq[i]; }
    }
    if (m == 0) return;
    if (m == 1) { len[ka[0] & 511u] = 1; return; }
    for (int sh = 9; sh < 32 && (maxf >> (sh - 9)) != 0; sh += 7) {
        for (int j = 0; j < 128; j++) cnt[j] = 0;
        for (int i = 0; i < m; i++) cnt[(ka[i] >> sh) & 127u]++;
        uint32_t at = 0;
        for (int j = 0; j < 128; j++) { const uint32_t c = cnt[j]; cnt[j] = at; at += c; }
        for (int i = 0; i < m; i++) kb[cnt[(ka[i] >> sh) & 127u]++] = ka[i];
        uint32_t *sw = ka; ka = kb; kb = sw;
    }
    uint32_t *A = kb;                                   // weights, then parents, then depths
    for (int i = 0; i < m; i++) A[i] = ka[i] >> 9;
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < m - 1; next++) {
        if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[m - 2] = 0;
    for (next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = m - 2; next = m - 1;
    while (avbl > 0) {                                  // one round per depth, at most m - 1
        while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
    for (int l = 0; l <= limit; l++) cnt[l] = 0;
    for (int i = 0; i < m; i++) cnt[(int)A[i] > limit ? limit : (int)A[i]]++;
    uint32_t total = 0;
    for (int l = limit; l > 0; l--) total += cnt[l] << (limit - l);
    for (int it = 0; it < m && total > (1u << limit); it++) {
        cnt[limit]--;
        for (int l = limit - 1; l > 0; l--)
            if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
        total--;
    }
    int i = 0;
    for (int l = limit; l > 0; l--)
        for (uint32_t c = 0; c < cnt[l]; c++) len[ka[i++] & 511u] = (uint8_t)l;
}
PNG_HD void png_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len)
{
    uint32_t ws[2 * PNG_NLL + 128];
    png_code_lengths_ws(freq, n, limit, len, ws);
}

// zlib's rule for fewer than two used distance symbols: give unused ones the frequency 1 until there are two -- the next after the
// highest used while that is below 2, else symbol 0 -- so that the distance set is complete in every block.  pad: the symbols it added, or -1
PNG_HD void png_dist_pad(uint32_t *df, int pad[2])
{
    int used = 0, maxc = -1;
    for (int i = 0; i < PNG_ND; i++) if (df[i]) { used++; maxc = i; }
    pad[0] = pad[1] = -1;
    for (int k = 0; used < 2; used++, k++) {
        const int node = maxc < 2 ? ++maxc : 0;
        df[node] = 1;
        pad[k] = node;
    }
}

// the order in which the code-length code's own lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
PNG_HD int png_cl_order(int i) { return (int)((i < 12 ? 0x22caa324e804a30ull >> (5 * i) : 0x3c2e1346cull >> (5 * (i - 12))) & 31); }

struct PngDyn {
    uint8_t ll_len[PNG_NLL], d_len[PNG_ND], cl_len[PNG_NCL];
    int hlit, hdist, hclen;     // trimmed counts: 257..286, 1..30, 4..19
    uint32_t hdr;               // bits in front of the first token: 3 + 14 + 3 hclen + the coded lengths
    uint32_t bits;              // the whole block: hdr, the tokens with their extra bits, the end of block
};

// One step of the run-length coding of the length sequence ll[0, hlit) ++ d[0, total - hlit) at i.  Greedy: v = the value at i, r = how
// often it stands there in a row (counted up to 138 for 0, up to 6 otherwise).  v = 0 and r >= 3: symbol 17 (r <= 10) or 18; v > 0, the
// value before i equal to v and r >= 3: symbol 16; else v itself, alone.  Returns how many lengths the symbol covers
PNG_HD int png_rle_step(const uint8_t *ll, int hlit, const uint8_t *d, int total, int i, int &sym, int &ext, int &val)
{
    const int v = i < hlit ? ll[i] : d[i - hlit];
    const int cap = v == 0 ? 138 : 6;
    int r = 1;
    while (i + r < total && r < cap && (i + r < hlit ? ll[i + r] : d[i + r - hlit]) == v) r++;
    if (v == 0 && r >= 3) {
        if (r <= 10) { sym = 17; ext = 3; val = r - 3; } else { sym = 18; ext = 7; val = r - 11; }
        return r;
    }
    if (v != 0 && i > 0 && (i - 1 < hlit ? ll[i - 1] : d[i - 1 - hlit]) == v && r >= 3) { sym = 16; ext = 2; val = r - 3; return r; }
    sym = v; ext = 0; val = 0;
    return 1;
}

// The dynamic block of a stripe from its histograms: llf[PNG_NLL] (the end of block counted once), df[PNG_ND] (padded here) and the total
// of the tokens' extra bits -> the three sets of code lengths, the trimmed counts and the exact size in bits.  ws: PNG_WS_WORDS words
PNG_HD void png_dyn_plan(const uint32_t *llf, uint32_t *df, uint32_t extra_bits, PngDyn &D, uint32_t *ws)
{
    int pad[2];
    png_dist_pad(df, pad);
    png_code_lengths_ws(llf, PNG_NLL, 15, D.ll_len, ws);
    png_code_lengths_ws(df, PNG_ND, 15, D.d_len, ws);
    int hlit = PNG_NLL, hdist = PNG_ND, hclen = PNG_NCL;
    while (hlit > 257 && !D.ll_len[hlit - 1]) hlit--;
    while (hdist > 1 && !D.d_len[hdist - 1]) hdist--;
    uint32_t *clf = ws + 2 * PNG_NLL + 128;
    for (int s = 0; s < PNG_NCL; s++) clf[s] = 0;
    uint32_t hdr = 3 + 14;
    for (int i = 0; i < hlit + hdist;) {
        int sym, ext, val;
        i += png_rle_step(D.ll_len, hlit, D.d_len, hlit + hdist, i, sym, ext, val);
        clf[sym]++;
        hdr += (uint32_t)ext;
    }
    png_code_lengths_ws(clf, PNG_NCL, 7, D.cl_len, ws);
    while (hclen > 4 && !D.cl_len[png_cl_order(hclen - 1)]) hclen--;
    hdr += 3u * (uint32_t)hclen;
    for (int s = 0; s < PNG_NCL; s++) hdr += clf[s] * D.cl_len[s];
    uint32_t bits = hdr + extra_bits;
    for (int s = 0; s < PNG_NLL; s++) bits += llf[s] * D.ll_len[s];
    for (int s = 0; s < PNG_ND; s++) bits += df[s] * D.d_len[s];
    for (int k = 0; k < 2; k++) if (pad[k] >= 0) bits -= D.d_len[pad[k]];
    D.hlit = hlit; D.hdist = hdist; D.hclen = hclen; D.hdr = hdr; D.bits = bits;
}

// canonical codes (RFC 1951 3.2.2) of the lengths len[0, n): code[s] = the code as it enters the stream | its length << 16, 0 for an
// unused symbol.  ws: 32 words
PNG_HD void png_canonical(const uint8_t *len, int n, uint32_t *code, uint32_t *ws)
{
    uint32_t *bl = ws, *nx = ws + 16;
    for (int b = 0; b < 16; b++) bl[b] = 0;
    for (int s = 0; s < n; s++) bl[len[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; b++) { c = (c + bl[b - 1]) << 1; nx[b] = c; }
    for (int s = 0; s < n; s++) {
        const int l = len[s];
        code[s] = l ? png_rev(nx[l]++, l) | ((uint32_t)l << 16) : 0u;
    }
}

// the header of a dynamic block, bit field after bit field through put(value, bits); clc: the canonical codes of D.cl_len
template <class Put>
PNG_HD void png_dyn_header(const PngDyn &D, const uint32_t *clc, bool last, Put &&put)
{
    put((last ? 1u : 0u) | 4u, 3);
    put((uint32_t)(D.hlit - 257), 5);
    put((uint32_t)(D.hdist - 1), 5);
    put((uint32_t)(D.hclen - 4), 4);
    for (int i = 0; i < D.hclen; i++) put(D.cl_len[png_cl_order(i)], 3);
    for (int i = 0; i < D.hlit + D.hdist;) {
        int sym, ext, val;
        i += png_rle_step(D.ll_len, D.hlit, D.d_len, D.hlit + D.hdist, i, sym, ext, val);
        put(clc[sym] & 0xffffu, (int)(clc[sym] >> 16));
        if (ext) put((uint32_t)val, ext);
    }
}

// one token of a dynamic block with the code tables llc, dc (png_canonical): v1 / bits1 (at most 20) the literal or the length with its
// extra bits, v2 / bits2 (at most 28, 0 for a literal) the distance with its
PNG_HD void png_dyn_token(const uint32_t *llc, const uint32_t *dc, int len, int dist, int lit, uint32_t &v1, int &bits1, uint32_t &v2, int &bits2)
{
    if (len == 0) { v1 = llc[lit] & 0xffffu; bits1 = (int)(llc[lit] >> 16); v2 = 0; bits2 = 0; return; }
    int lcode, lext, lval, dcode, dext, dval;
    png_len_sym(len, lcode, lext, lval);
    png_dist_sym(dist, dcode, dext, dval);
    const uint32_t a = llc[257 + lcode], b = dc[dcode];
    bits1 = (int)(a >> 16); v1 = (a & 0xffffu) | ((uint32_t)lval << bits1); bits1 += lext;
    bits2 = (int)(b >> 16); v2 = (b & 0xffffu) | ((uint32_t)dval << bits2); bits2 += dext;
}

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
void png_encode_host(const uint8_t *pic, const PngShape &g, int mode, uint8_t *out, size_t *size);

#ifdef __HIPCC__
// ---- device (png_kernels.hip): k pictures of shape g at pics -> k files at files + i fcap, file_size[i] bytes each.
// filt: k g.raw bytes, slots: k g.ns PNG_SLOT bytes, meta: 4 k g.ns words, file_size: k words; fcap >= g.bound; mode: PNG_FAST or
// PNG_COMPACT.  0 on success.
int png_encode_launch(const uint8_t *pics, int k, const PngShape &g, int mode, uint8_t *filt, uint8_t *slots, uint32_t *meta, uint8_t *files, size_t fcap,
                      uint32_t *file_size, hipStream_t s);
// png_code_lengths for k histograms of n symbols in device memory, one lane each (tmat_debug_png_code_lengths).  0 on success.
int png_code_lengths_launch(const uint32_t *freqs, int k, int n, int limit, uint8_t *lens, hipStream_t s);
// n pictures (host or device memory) through the handle's stream and pool, in the handle's mode (tmat_png_set_mode), in chunks that bound device memory: file i at
// out + i cap_each (host), sizes[i] its length; cap_each >= g.bound.  ms3 (nullable): += HIP-event ms of {upload, kernels, copy back}.
// Returns a TMAT_* code.  (tmat_api.cpp)
struct Ctx;
int png_encode_ctx(Ctx *c, const uint8_t *pics, bool on_host, int n, const PngShape &g, uint8_t *out, size_t cap_each, size_t *sizes, float *ms3);
#endif

}  // namespace tmat
