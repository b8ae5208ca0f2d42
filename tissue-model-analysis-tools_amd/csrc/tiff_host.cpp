// TIFF input (tiff.h): the container parser, the plan of a decode call and the host twin of the device decoder.  No GPU,
// no handle; nothing here trusts the file: every offset, count and product is checked against the file's size before it is used.
#include "tiff.h"

#include <algorithm>
#include <unordered_set>

namespace tmat {

namespace {

struct Reader {
    const uint8_t *f;
    size_t n;
    bool be;
    bool has(uint64_t off, uint64_t len) const { return off <= n && len <= n - off; }
    uint32_t u16(size_t o) const { return be ? ((uint32_t)f[o] << 8) | f[o + 1] : (uint32_t)f[o] | ((uint32_t)f[o + 1] << 8); }
    uint32_t u32(size_t o) const
    {
        return be ? ((uint32_t)f[o] << 24) | ((uint32_t)f[o + 1] << 16) | ((uint32_t)f[o + 2] << 8) | f[o + 3]
                  : (uint32_t)f[o] | ((uint32_t)f[o + 1] << 8) | ((uint32_t)f[o + 2] << 16) | ((uint32_t)f[o + 3] << 24);
    }
};

struct Tag {
    bool present = false;
    uint32_t type = 0, count = 0;
    size_t at = 0;          // where its values lie (inside the entry or out of line), checked
};

// the values of a SHORT / LONG tag lie inside the file: fills t.at.  false: a type or position that cannot be read
bool locate(const Reader &r, size_t entry, Tag &t)
{
    t.present = true;
    t.type = r.u16(entry + 2);
    t.count = r.u32(entry + 4);
    if ((t.type != 3 && t.type != 4) || t.count < 1) return false;
    const uint64_t bytes = (uint64_t)t.count * (t.type == 3 ? 2 : 4);
    if (bytes <= 4) { t.at = entry + 8; return true; }
    const uint32_t off = r.u32(entry + 8);
    if (!r.has(off, bytes)) return false;
    t.at = off;
    return true;
}
uint32_t value(const Reader &r, const Tag &t, uint32_t i) { return t.type == 3 ? r.u16(t.at + 2 * (size_t)i) : r.u32(t.at + 4 * (size_t)i); }

// one IFD at `ifd` (entry count already known to fit): the page, and its strips when asked
void parse_page(const Reader &r, size_t ifd, uint32_t n_entries, TiffPageInfo &p, std::vector<std::pair<uint32_t, uint32_t>> *strips)
{
    p = TiffPageInfo{};
    p.big_endian = r.be;
    p.status = TIFF_CORRUPT;
    p.reason = TIFF_R_TAG;
    enum { W, H, BPS, COMP, PHOTO, FILL, OFFS, SPP, RPS, CNTS, PLANAR, PRED, TILEW, TILEL, TILEO, SFMT, N_TAGS };
    static const uint32_t ids[N_TAGS] = {256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 322, 323, 324, 339};
    Tag tag[N_TAGS];
    for (uint32_t e = 0; e < n_entries; e++) {
        const size_t entry = ifd + 2 + 12 * (size_t)e;
        const uint32_t id = r.u16(entry);
        for (int k = 0; k < N_TAGS; k++)
            if (ids[k] == id && !tag[k].present && !locate(r, entry, tag[k])) return;
    }
    auto scalar = [&](int k, uint32_t dflt) { return tag[k].present ? value(r, tag[k], 0) : dflt; };
    if (!tag[W].present || !tag[H].present) return;
    const uint32_t w = scalar(W, 0), h = scalar(H, 0);
    if (w < 1 || h < 1 || w > 0x7fffffffu || h > 0x7fffffffu) return;
    p.width = (int32_t)w; p.height = (int32_t)h;
    const uint32_t bps = scalar(BPS, 1), comp = scalar(COMP, 1), pred = scalar(PRED, 1), spp = scalar(SPP, 1);
    p.bits = (int32_t)std::min<uint32_t>(bps, 0x7fffffffu);
    p.compression = (int32_t)comp;
    p.predictor = (int32_t)pred;
    auto fallback = [&](int why) { p.status = TIFF_FALLBACK; p.reason = why; };
    if (tag[TILEW].present || tag[TILEL].present || tag[TILEO].present) return fallback(TIFF_R_TILES);
    if (spp != 1) return fallback(TIFF_R_SAMPLES);
    if (bps != 8 && bps != 16) return fallback(TIFF_R_BITS);
    if (scalar(SFMT, 1) != 1) return fallback(TIFF_R_SAMPLE_FORMAT);
    if (scalar(PHOTO, 0xffffffffu) != 1) return fallback(TIFF_R_PHOTOMETRIC);
    if (scalar(FILL, 1) != 1) return fallback(TIFF_R_FILL_ORDER);
    if (scalar(PLANAR, 1) != 1) return fallback(TIFF_R_PLANAR);
    if (comp != TIFF_COMP_NONE && comp != TIFF_COMP_LZW && comp != TIFF_COMP_PACKBITS) return fallback(TIFF_R_COMPRESSION);
    if (pred != 1 && !(pred == 2 && comp == TIFF_COMP_LZW)) return fallback(TIFF_R_PREDICTOR);
    const uint64_t row_bytes = (uint64_t)w * (bps / 8), plane_bytes = row_bytes * h;
    if (plane_bytes > TIFF_MAX_PLANE_BYTES) return fallback(TIFF_R_SIZE);
    // strips
    p.reason = TIFF_R_STRIPS;
    if (!tag[OFFS].present || !tag[CNTS].present) return;
    uint32_t rps = scalar(RPS, 0xffffffffu);
    if (rps < 1) return;
    rps = std::min(rps, h);
    const uint32_t ns = (h + rps - 1) / rps;
    p.rows_per_strip = (int32_t)rps;
    p.n_strips = (int32_t)ns;
    if (tag[OFFS].count != ns || tag[CNTS].count != ns) return;
    for (uint32_t i = 0; i < ns; i++) {                     // ns values lie inside the file (locate), so ns is bounded by its size
        const uint32_t off = value(r, tag[OFFS], i), cnt = value(r, tag[CNTS], i);
        if (!r.has(off, cnt) || cnt < 1) return;
        const uint64_t rows = i + 1 < ns ? rps : h - (uint64_t)rps * (ns - 1);
        if (comp == TIFF_COMP_NONE && cnt < rows * row_bytes) return;
    }
    if (comp == TIFF_COMP_LZW) {                            // libtiff's test for the old-style (LSB-first) LZW streams
        const uint32_t off = value(r, tag[OFFS], 0), cnt = value(r, tag[CNTS], 0);
        if (cnt >= 2 && r.f[off] == 0 && (r.f[off + 1] & 1)) return fallback(TIFF_R_OLD_LZW);
    }
    p.status = TIFF_OK;
    p.reason = TIFF_R_NONE;
    if (strips) {
        strips->resize(ns);
        for (uint32_t i = 0; i < ns; i++) (*strips)[i] = {value(r, tag[OFFS], i), value(r, tag[CNTS], i)};
    }
}

}  // namespace

void tiff_walk(const uint8_t *file, size_t n, int cap_pages, TiffPageInfo *pages, int *n_pages, int strips_of,
               std::vector<std::pair<uint32_t, uint32_t>> *strips)
{
    int count = 0;
    auto put = [&](const TiffPageInfo &p) { if (count < cap_pages) pages[count] = p; count++; };
    auto stop = [&](int status, int reason) {
        TiffPageInfo p{};
        p.status = status; p.reason = reason;
        put(p);
        *n_pages = count;
    };
    if (n < 8 || !((file[0] == 'I' && file[1] == 'I') || (file[0] == 'M' && file[1] == 'M'))) return stop(TIFF_CORRUPT, TIFF_R_HEADER);
    const Reader r{file, n, file[0] == 'M'};
    const uint32_t magic = r.u16(2);
    if (magic == 43) return stop(TIFF_FALLBACK, TIFF_R_BIGTIFF);
    if (magic != 42) return stop(TIFF_CORRUPT, TIFF_R_HEADER);
    std::unordered_set<uint32_t> seen;
    uint32_t ifd = r.u32(4);
    if (ifd == 0) return stop(TIFF_CORRUPT, TIFF_R_IFD);
    while (ifd != 0) {                                      // every turn visits a new offset of a bounded file
        if (!seen.insert(ifd).second) return stop(TIFF_CORRUPT, TIFF_R_LOOP);
        if (ifd < 8 || !r.has(ifd, 2)) return stop(TIFF_CORRUPT, TIFF_R_IFD);
        const uint32_t n_entries = r.u16(ifd);
        if (!r.has((uint64_t)ifd + 2, 12 * (uint64_t)n_entries + 4)) return stop(TIFF_CORRUPT, TIFF_R_IFD);
        TiffPageInfo p;
        parse_page(r, ifd, n_entries, p, count == strips_of ? strips : nullptr);
        put(p);
        if (count - 1 == strips_of) break;
        ifd = r.u32((size_t)ifd + 2 + 12 * (size_t)n_entries);
    }
    *n_pages = count;
}

bool tiff_plan(const uint8_t *const *files, const size_t *n_bytes, const int *file_of, const int *page_of, int n_planes, int H, int W,
               TiffPlan &plan, int *status, std::string &err)
{
    plan.planes.assign((size_t)n_planes, TiffPlane{});
    plan.strips.clear();
    plan.bits = 0;
    std::vector<std::pair<uint32_t, uint32_t>> strips;
    std::vector<TiffPageInfo> pages;
    for (int i = 0; i < n_planes; i++) {
        TiffPlane &pl = plan.planes[(size_t)i];
        pl.out_index = i;
        const int page = page_of[i];
        const uint8_t *f = files[file_of[i]];
        int np = 0;
        status[i] = TIFF_CORRUPT;
        if (page < 0 || !f) continue;
        pages.assign((size_t)page + 1, TiffPageInfo{});
        tiff_walk(f, n_bytes[file_of[i]], page + 1, pages.data(), &np, page, &strips);
        if (np < page + 1) {                               // the chain ended, or broke, before this page
            if (np > 0 && pages[(size_t)np - 1].status == TIFF_FALLBACK && pages[(size_t)np - 1].reason == TIFF_R_BIGTIFF) status[i] = TIFF_FALLBACK;
            continue;
        }
        const TiffPageInfo &p = pages[(size_t)page];
        status[i] = p.status;
        if (p.status != TIFF_OK) continue;
        if (p.width != W || p.height != H) { err = "a supported plane is not of the call's shape (H, W)"; return false; }
        if (plan.bits && plan.bits != p.bits) { err = "the supported planes differ in bit depth"; return false; }
        plan.bits = p.bits;
        pl.ok = 1;
        pl.first_strip = (int32_t)plan.strips.size();
        pl.rps = p.rows_per_strip;
        pl.comp = p.compression;
        pl.bytes = p.bits / 8;
        pl.swap = p.big_endian;
        pl.predictor = p.predictor;
        const uint64_t row_bytes = (uint64_t)W * (uint64_t)pl.bytes;
        for (int s = 0; s < p.n_strips; s++) {
            const int rows = std::min(p.rows_per_strip, H - s * p.rows_per_strip);
            TiffStrip st{};
            st.src = strips[(size_t)s].first;
            st.n_in = strips[(size_t)s].second;
            st.dst = (uint64_t)s * (uint64_t)p.rows_per_strip * row_bytes;
            st.n_out = (uint32_t)((uint64_t)rows * row_bytes);
            st.plane = i;
            st.comp = p.compression;
            plan.strips.push_back(st);
        }
    }
    return true;
}

void tiff_decode_host(const uint8_t *const *files, const int *file_of, const TiffPlan &plan, int H, int W, uint16_t *out, int *status)
{
    std::vector<uint8_t> raw;
    std::vector<uint32_t> table(TIFF_LZW_SIZE);
    for (size_t i = 0; i < plan.planes.size(); i++) {
        const TiffPlane &pl = plan.planes[i];
        if (!pl.ok) continue;
        const uint8_t *file = files[file_of[i]];
        const int n_strips = (H + pl.rps - 1) / pl.rps;
        bool good = true;
        if (pl.comp != TIFF_COMP_NONE) {
            raw.assign((size_t)H * W * pl.bytes, 0);
            for (int s = 0; s < n_strips && good; s++) {
                const TiffStrip &st = plan.strips[(size_t)pl.first_strip + s];
                good = tiff_strip_decode(st.comp, file + st.src, st.n_in, raw.data() + st.dst, st.n_out, table.data()) == TIFF_OK;
            }
        }
        if (!good) { status[i] = TIFF_CORRUPT; continue; }
        uint16_t *o = out + (size_t)pl.out_index * H * W;
        for (int y = 0; y < H; y++) {
            const uint8_t *row = tiff_row(pl, plan.strips.data(), file, raw.data(), y, W);
            uint32_t acc = 0;
            for (int x = 0; x < W; x++) {
                const uint32_t v = tiff_sample(row, x, pl.bytes, pl.swap);
                acc = pl.predictor == 2 ? acc + v : v;
                o[(size_t)y * W + x] = tiff_widen(acc, pl.bytes);
            }
        }
    }
}

}  // namespace tmat
