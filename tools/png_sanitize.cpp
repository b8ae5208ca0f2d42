// Stand-alone sanitizer run of the PNG encoder's host twin (csrc/png_host.cpp alone: no GPU, no Python): both modes over the shapes and
// contents of tests/helpers/png_check.py, every output buffer of exactly tmat_png_bound bytes on the heap, so that a byte past the bound
// is a report; then png_code_lengths over steep and flat histograms.  Build and run (any C++17 compiler):
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I tissue-model-analysis-tools_amd/csrc \
//       tools/png_sanitize.cpp tissue-model-analysis-tools_amd/csrc/png_host.cpp -o png_sanitize && ./png_sanitize
#include "png.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace tmat;

static std::vector<uint8_t> content(int kind, int H, int W, int ch)
{
    std::vector<uint8_t> p((size_t)H * W * ch);
    uint32_t lcg = 12345u + (uint32_t)kind;
    uint8_t pat[300];
    for (uint8_t &v : pat) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)(lcg >> 24); }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            for (int c = 0; c < ch; c++) {
                const size_t i = ((size_t)y * W + x) * ch + c;
                int v = 0;
                switch (kind) {
                case 0: v = 200; break;
                case 1: v = x * 3 + c; break;
                case 2: v = y * 5 + c; break;
                case 3: lcg = lcg * 1664525u + 1013904223u; v = (int)(lcg >> 24); break;
                case 4: v = (std::pow((y - 0.45 * H) / std::fmax(1.0, 0.3 * H), 2) + std::pow((x - 0.55 * W) / std::fmax(1.0, 0.25 * W), 2) < 1.0) ? 255 : 0; break;
                case 5: v = (int)(127 + 100 * std::sin((y + 7 * c) / 17.0) * std::cos(x / 23.0)); break;
                default: v = pat[i % 300]; break;
                }
                p[i] = (uint8_t)v;
            }
    return p;
}

int main()
{
    const int S = PNG_STRIPE;
    const int shapes[][3] = {{1, 1, 1}, {1, 1, 3}, {1, 7, 1}, {7, 1, 1}, {33, 31, 3}, {401, 37, 1}, {1, S - 2, 1}, {2, S / 2 - 1, 1}, {1, S, 1}, {1, 2 * S, 1},
                             {1, 70000, 1}, {640, 640, 1}, {300, 300, 3}};
    size_t files = 0, bytes[2] = {0, 0};
    for (const auto &sh : shapes)
        for (int kind = 0; kind < 7; kind++) {
            PngShape g;
            if (!png_shape(sh[0], sh[1], sh[2], g)) { std::printf("bad shape\n"); return 1; }
            const std::vector<uint8_t> pic = content(kind, sh[0], sh[1], sh[2]);
            size_t size[2];
            for (int mode = 0; mode < 2; mode++) {
                uint8_t *out = (uint8_t *)std::malloc(g.bound);         // exactly the bound
                png_encode_host(pic.data(), g, mode, out, &size[mode]);
                std::free(out);
                if (size[mode] > g.bound || size[mode] < (size_t)PNG_HEAD + PNG_TAIL) { std::printf("size outside its range\n"); return 1; }
                bytes[mode] += size[mode];
                files++;
            }
            if (size[PNG_COMPACT] > size[PNG_FAST]) { std::printf("compact larger than fast: %d x %d x %d, kind %d\n", sh[0], sh[1], sh[2], kind); return 1; }
        }
    // code lengths: Fibonacci (deeper than the limit), geometric, flat, sparse
    int sets = 0;
    for (int limit : {15, 7})
        for (int variant = 0; variant < 40; variant++) {
            const int nmax = limit == 15 ? PNG_NLL : PNG_NCL, n = 2 + (variant * 37) % (nmax - 1);
            std::vector<uint32_t> f(n);
            uint32_t a = 1, b = 1;
            for (int i = 0; i < n; i++) {
                if (variant % 4 == 0) { f[i] = a; const uint32_t c = a + b; a = b; b = c < (1u << 14) ? c : 1; }
                else if (variant % 4 == 1) f[i] = 1 + (uint32_t)(i * 7919 % 13);
                else if (variant % 4 == 2) f[i] = i % 3 ? 0 : 1u << (i % 15);
                else f[i] = 5;
            }
            f[0] += 1; f[n - 1] += 1;
            std::vector<uint8_t> len(n);                              // exactly n
            png_code_lengths(f.data(), n, limit, len.data());
            uint64_t kraft = 0;
            int used = 0;
            for (int i = 0; i < n; i++) {
                if ((len[i] == 0) != (f[i] == 0) || len[i] > limit) { std::printf("bad length\n"); return 1; }
                if (len[i]) { kraft += 1ull << (limit - len[i]); used++; }
            }
            if (used > 1 && kraft != 1ull << limit) { std::printf("Kraft sum off: limit %d variant %d\n", limit, variant); return 1; }
            sets++;
        }
    std::printf("png_sanitize: %zu files (fast %zu bytes, compact %zu bytes), %d sets of code lengths, clean\n", files, bytes[0], bytes[1], sets);
    return 0;
}
