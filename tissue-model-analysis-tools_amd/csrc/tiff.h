// TIFF decoder: every rule of the strip streams, shared by tiff_host.cpp (container parsing and the host twin) and
// tiff_kernels.hip (device), which must produce the same pixels.  A plane is one page of one classic TIFF file, cut into strips; a
// strip is decoded on its own into `rows x W x bytes` raw bytes, then the rows are finished:
//   LZW       codes MSB first, 9 to 12 bits; Clear 256, EOI 257, first free entry 258.  The width grows when the next free entry
//             equals (1 << width) - 1 (TIFF's early change), never beyond 12.  The first code after Clear is a literal.  A code equal
//             to the next free entry is the previous string plus its first byte (KwKwK); a code above it is corrupt.  Entries stop
//             being added at 4096 and decoding goes on.  Decoding stops when the strip's byte count is produced, whether or not EOI
//             follows (a string that would pass the count is cut there); EOI or the end of the input before that is corrupt.
//   PackBits  control n in [0, 127]: n + 1 literals; n in [-127, -1]: the next byte 1 - n times; -128: nothing.  Decoding stops at the
//             strip's byte count; a run or a literal block that would pass it, or the end of the input before it, is corrupt.
//   rows      decode, then byte-swap 16-bit samples of MM files, then predictor 2 as a running sum per row modulo 2^bits, then widen
//             to uint16.
// A table entry is (prefix code, last byte, length) in 32 bits; a string is written back to front by walking the prefixes, so the
// decoder never reads its own output.  Every loop is bounded by the strip's input or output size, every store is inside
// out[0, n_out), every table index is checked before use, a read past the input yields zero bits and the corrupt status.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define TIFF_HD __host__ __device__ inline
#else
#define TIFF_HD inline
#endif

namespace tmat {

constexpr int TIFF_OK = 0, TIFF_FALLBACK = 1, TIFF_CORRUPT = 2;        // TMAT_TIFF_OK, TMAT_TIFF_FALLBACK, TMAT_TIFF_CORRUPT
constexpr int TIFF_COMP_NONE = 1, TIFF_COMP_LZW = 5, TIFF_COMP_PACKBITS = 32773;
constexpr int TIFF_LZW_CLEAR = 256, TIFF_LZW_EOI = 257, TIFF_LZW_FIRST = 258, TIFF_LZW_SIZE = 4096, TIFF_LZW_MAXBITS = 12;
constexpr size_t TIFF_MAX_PLANE_BYTES = (size_t)1 << 30;                // H W bytes of one plane, and so of one strip's output

// one strip of one plane of a call: where its bytes lie in the uploaded files, and where its raw rows go
struct TiffStrip {
    uint64_t src;       // first byte, from the start of its file
    uint64_t dst;       // first raw byte, from the start of its plane's raw bytes (uncompressed strips are read in place)
    uint32_t n_in;      // compressed bytes
    uint32_t n_out;     // raw bytes: rows * W * bytes
    int32_t plane;      // index into the call's planes
    int32_t comp;       // TIFF_COMP_*
};

// one plane of a call, for the row kernels
struct TiffPlane {
    uint64_t raw;           // its first byte in the raw buffer (compressed planes)
    uint64_t file_base;     // its file's first byte in the file blob
    int32_t first_strip;    // index of its strip 0
    int32_t rps;            // rows per strip
    int32_t comp, bytes, swap, predictor;
    int32_t ok;             // 0: not decoded (fallback, corrupt container): no kernel touches it
    int32_t out_index;      // which (H, W) slice of the output it fills
};

// ---- LZW ----

TIFF_HD uint32_t tiff_lzw_entry(int prefix, int last, int len) { return (uint32_t)prefix | ((uint32_t)last << 12) | ((uint32_t)len << 20); }
TIFF_HD int tiff_lzw_prefix(uint32_t e) { return (int)(e & 0xfffu); }
TIFF_HD int tiff_lzw_last(uint32_t e) { return (int)((e >> 12) & 0xffu); }
TIFF_HD int tiff_lzw_len(uint32_t e) { return (int)(e >> 20); }

// the next four bytes of in[pos, n) as a big-endian word; bytes past n read as zero
TIFF_HD uint32_t tiff_be32(const uint8_t *in, size_t n, size_t pos)
{
    if (pos + 4 <= n) {
        uint32_t w;
        __builtin_memcpy(&w, in + pos, 4);
        return __builtin_bswap32(w);
    }
    uint32_t w = 0;
    for (int k = 0; k < 4; k++) w = (w << 8) | (pos + k < n ? in[pos + k] : 0u);
    return w;
}

// MSB-first bit reader over in[0, n).  `ahead` is the word after the ones in `acc`, loaded one refill early so that its latency
// overlaps the codes in between.
struct TiffBits {
    const uint8_t *in;
    size_t n, pos;          // pos: first byte not yet in acc or ahead
    uint64_t acc;           // next bits at the top
    int have;               // valid bits in acc
    uint64_t used;          // bits handed out
    uint32_t ahead;
};
TIFF_HD void tiff_bits_open(TiffBits &b, const uint8_t *in, size_t n)
{
    b.in = in; b.n = n; b.used = 0;
    b.acc = ((uint64_t)tiff_be32(in, n, 0) << 32) | tiff_be32(in, n, 4);
    b.have = 64;
    b.ahead = tiff_be32(in, n, 8);
    b.pos = 12;
}
// the next `width` bits (9 to 12); past the input they are zero, and tiff_bits_overrun says so
TIFF_HD int tiff_bits_get(TiffBits &b, int width)
{
    const int code = (int)(b.acc >> (64 - width));
    b.acc <<= width;
    b.have -= width;
    b.used += (uint64_t)width;
    if (b.have <= 32) {
        b.acc |= (uint64_t)b.ahead << (32 - b.have);
        b.have += 32;
        b.ahead = b.pos < b.n ? tiff_be32(b.in, b.n, b.pos) : 0u;
        b.pos += 4;
    }
    return code;
}
TIFF_HD bool tiff_bits_overrun(const TiffBits &b) { return b.used > (uint64_t)b.n * 8u; }

// One LZW strip: in[0, n_in) -> out[0, n_out).  table: TIFF_LZW_SIZE words of scratch, nothing assumed about its contents (an entry
// is written before any code may name it).  TIFF_OK or TIFF_CORRUPT.
TIFF_HD int tiff_lzw_decode(const uint8_t *in, size_t n_in, uint8_t *out, size_t n_out, uint32_t *table)
{
    TiffBits b;
    tiff_bits_open(b, in, n_in);
    int width = 9, free_ent = TIFF_LZW_FIRST, prev = -1, prev_first = 0;
    size_t pos = 0;
    while (pos < n_out) {                                   // every turn consumes at least 9 bits of a bounded input
        const int code = tiff_bits_get(b, width);
        if (tiff_bits_overrun(b) || code == TIFF_LZW_EOI) return TIFF_CORRUPT;
        if (code == TIFF_LZW_CLEAR) { width = 9; free_ent = TIFF_LZW_FIRST; prev = -1; continue; }
        if (prev < 0) {                                     // first code of the strip or after Clear: a literal
            if (code > 255) return TIFF_CORRUPT;
            out[pos++] = (uint8_t)code;
            prev = code; prev_first = code;
            continue;
        }
        if (code > free_ent || (code == free_ent && free_ent >= TIFF_LZW_SIZE)) return TIFF_CORRUPT;
        const int prev_len = prev < 256 ? 1 : tiff_lzw_len(table[prev]);
        const bool kwkwk = code == free_ent;
        if (kwkwk) table[free_ent] = tiff_lzw_entry(prev, prev_first, prev_len + 1);
        // write the string of `code` back to front; bytes past n_out are dropped
        const int len = code < 256 ? 1 : tiff_lzw_len(table[code]);
        int c = code, first = 0;
        for (int t = len - 1; t >= 0; t--) {                // at most `len` <= 4095 steps whatever the table holds
            int byte;
            if (c < 256) { byte = c; first = c; if (t != 0) return TIFF_CORRUPT; }
            else {
                if (c < TIFF_LZW_FIRST || c >= TIFF_LZW_SIZE || t == 0) return TIFF_CORRUPT;
                const uint32_t e = table[c];
                byte = tiff_lzw_last(e);
                c = tiff_lzw_prefix(e);
            }
            if (pos + (size_t)t < n_out) out[pos + (size_t)t] = (uint8_t)byte;
        }
        pos += (size_t)len;
        if (free_ent < TIFF_LZW_SIZE) {
            if (!kwkwk) table[free_ent] = tiff_lzw_entry(prev, first, prev_len + 1);
            free_ent++;
            if (free_ent == (1 << width) - 1 && width < TIFF_LZW_MAXBITS) width++;
        }
        prev = code; prev_first = first;
    }
    return TIFF_OK;
}

// ---- PackBits ----

TIFF_HD int tiff_packbits_decode(const uint8_t *in, size_t n_in, uint8_t *out, size_t n_out)
{
    size_t ip = 0, op = 0;
    while (op < n_out) {                                    // every turn consumes at least one input byte
        if (ip >= n_in) return TIFF_CORRUPT;
        const int n = (int8_t)in[ip++];
        if (n == -128) continue;
        if (n >= 0) {
            const size_t cnt = (size_t)n + 1;
            if (cnt > n_in - ip || cnt > n_out - op) return TIFF_CORRUPT;
            for (size_t k = 0; k < cnt; k++) out[op + k] = in[ip + k];
            ip += cnt; op += cnt;
        } else {
            const size_t cnt = (size_t)(1 - n);
            if (ip >= n_in || cnt > n_out - op) return TIFF_CORRUPT;
            const uint8_t v = in[ip++];
            for (size_t k = 0; k < cnt; k++) out[op + k] = v;
            op += cnt;
        }
    }
    return TIFF_OK;
}

TIFF_HD int tiff_strip_decode(int comp, const uint8_t *in, size_t n_in, uint8_t *out, size_t n_out, uint32_t *table)
{
    return comp == TIFF_COMP_LZW ? tiff_lzw_decode(in, n_in, out, n_out, table) : tiff_packbits_decode(in, n_in, out, n_out);
}

// ---- rows ----

// sample x of a raw row: 8-bit, or 16-bit in the file's byte order
TIFF_HD uint32_t tiff_sample(const uint8_t *row, int x, int bytes, int swap)
{
    if (bytes == 1) return row[x];
    const uint32_t lo = row[2 * x], hi = row[2 * x + 1];
    return swap ? (lo << 8) | hi : lo | (hi << 8);
}
// the value stored for a sample whose running sum (or itself, without the predictor) is acc
TIFF_HD uint16_t tiff_widen(uint32_t acc, int bytes) { return (uint16_t)(bytes == 1 ? acc & 0xffu : acc & 0xffffu); }

// the start of row y of a plane: in the file for an uncompressed plane, in the raw buffer otherwise
TIFF_HD const uint8_t *tiff_row(const TiffPlane &p, const TiffStrip *strips, const uint8_t *file, const uint8_t *raw, int y, int W)
{
    const TiffStrip &s = strips[p.first_strip + y / p.rps];
    const size_t in_strip = (size_t)(y % p.rps) * (size_t)W * (size_t)p.bytes;
    return p.comp == TIFF_COMP_NONE ? file + s.src + in_strip : raw + s.dst + in_strip;
}

}  // namespace tmat

// ---- container and plan (tiff_host.cpp; host only) ----
#include <string>
#include <vector>

namespace tmat {

// reasons of tmat_tiff_page.reason (TMAT_TIFF_R_*)
enum {
    TIFF_R_NONE = 0, TIFF_R_HEADER = 1, TIFF_R_IFD = 2, TIFF_R_LOOP = 3, TIFF_R_TAG = 4, TIFF_R_STRIPS = 5, TIFF_R_STREAM = 6, TIFF_R_PAGE = 7,
    TIFF_R_BIGTIFF = 20, TIFF_R_TILES = 21, TIFF_R_SAMPLES = 22, TIFF_R_BITS = 23, TIFF_R_SAMPLE_FORMAT = 24, TIFF_R_PHOTOMETRIC = 25,
    TIFF_R_FILL_ORDER = 26, TIFF_R_PLANAR = 27, TIFF_R_COMPRESSION = 28, TIFF_R_PREDICTOR = 29, TIFF_R_OLD_LZW = 30, TIFF_R_SIZE = 31
};

struct TiffPageInfo {               // tmat_tiff_page, field for field
    int32_t width, height, bits, compression, predictor, big_endian, rows_per_strip, n_strips, status, reason;
};

// Walk the IFD chain of file[0, n): pages[0, min(cap_pages, *n_pages)) are filled.  Damage to the header or the chain ends the walk
// with one last page of status TIFF_CORRUPT.  strips_of >= 0: the (offset, byte count) pairs of that page, if its status is TIFF_OK.
void tiff_walk(const uint8_t *file, size_t n, int cap_pages, TiffPageInfo *pages, int *n_pages, int strips_of,
               std::vector<std::pair<uint32_t, uint32_t>> *strips);

// What a decode call does, worked out on the host from the containers alone: shared by the host twin and the device path.
struct TiffPlan {
    std::vector<TiffPlane> planes;      // one per plane of the call, in the caller's order; file_base and raw are left 0
    std::vector<TiffStrip> strips;      // of the planes with ok = 1; src is relative to the file, dst to the plane's raw bytes
    int bits = 0;                       // of the ok planes; 0 when there is none
};
// status[i] per plane; false (err set) when the ok planes disagree with (H, W) or among themselves in bit depth
bool tiff_plan(const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of, int n_planes, int H, int W,
               TiffPlan &plan, int *status, std::string &err);

// the host twin: decode the plan's planes into out (n_planes, H, W); a plane whose stream is corrupt gets TIFF_CORRUPT and is not written
void tiff_decode_host(const uint8_t *const *files, const int *file_of, const TiffPlan &plan, int H, int W, uint16_t *out, int *status);

#ifdef __HIPCC__
// tiff_kernels.hip: decode the strips [0, n_strips) and finish the rows of the planes [0, n_planes) of one chunk, all pointers device.
// bad: one int per plane, zeroed here, set by a corrupt strip; such a plane's output slice is not written.  0, or nonzero after a
// failed launch.
int tiff_decode_launch(const uint8_t *blob, const TiffStrip *strips, int n_strips, const TiffPlane *planes, int n_planes, int H, int W,
                       uint8_t *raw, uint16_t *out, int *bad, hipStream_t s);
// the plan's planes through the handle's stream and pool, in chunks that bound device memory: out is (n_planes, H, W) uint16 in host
// or device memory; status[i] becomes TIFF_CORRUPT for a plane whose stream is.  ms2 (nullable): += HIP-event ms of {upload, kernels}.
// Returns a TMAT_* code.  (tmat_api.cpp)
struct Ctx;
int tiff_decode_ctx(Ctx *c, const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const TiffPlan &plan, int H, int W,
                    uint16_t *out, bool out_on_host, int *status, float *ms2);
#endif

}  // namespace tmat
