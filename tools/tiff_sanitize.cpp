// Stand-alone sanitizer run of the TIFF parser and the decoder's host twin (csrc/tiff_host.cpp alone over csrc/tiff.h: no GPU, no
// Python).  It reads the fixtures of tests/helpers/tiff_files.py from a directory -- valid, unsupported and corrupt -- and decodes each
// into a heap buffer of exactly the plane's size with the file itself in a heap block of exactly its size, so that a byte read or
// written past either is a report.  Every file below 4 KiB is then decoded again at every truncation and with every byte replaced by
// 0x00, 0xff and its complement.  Build and run (any C++17 compiler):
//   python tests/helpers/tiff_files.py /tmp/tiff_fixtures
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I tissue-model-analysis-tools_amd/csrc \
//       tools/tiff_sanitize.cpp tissue-model-analysis-tools_amd/csrc/tiff_host.cpp -o tiff_sanitize && ./tiff_sanitize /tmp/tiff_fixtures
// The manifest (manifest.txt) has one line per case: file name, page, H, W, expected status (0 ok, 1 fallback, 2 corrupt) and, for an ok
// plane, the name of a file with its (H, W) uint16 pixels as Pillow decoded them.
#include "tiff.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

using namespace tmat;

static bool slurp(const std::string &path, uint8_t *&data, size_t &n)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    n = s.size();
    data = (uint8_t *)std::malloc(n ? n : 1);       // exactly the file
    std::memcpy(data, s.data(), n);
    return true;
}

// probe and decode one plane of file[0, n) into a buffer of exactly H W uint16; -> status, or -1 for TMAT_E_ARG-like refusals
static int decode(const uint8_t *file, size_t n, int page, int H, int W, uint16_t *out)
{
    int np = 0;
    TiffPageInfo pages[4];
    tiff_walk(file, n, 4, pages, &np, -1, nullptr);
    TiffPlan plan;
    std::string err;
    int status = -1, file_of = 0;
    const uint8_t *files[1] = {file};
    if (!tiff_plan(files, &n, &file_of, &page, 1, H, W, plan, &status, err)) return -1;
    tiff_decode_host(files, &file_of, plan, H, W, out, &status);
    return status;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: tiff_sanitize FIXTURE_DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::ifstream man(dir + "/manifest.txt");
    if (!man) { std::printf("no manifest in %s\n", dir.c_str()); return 2; }
    std::string line;
    size_t cases = 0, mutated = 0, by_status[3] = {0, 0, 0};
    while (std::getline(man, line)) {
        std::istringstream in(line);
        std::string name, pixels;
        int page, H, W, expect;
        if (!(in >> name >> page >> H >> W >> expect)) continue;
        in >> pixels;
        uint8_t *file = nullptr;
        size_t n = 0;
        if (!slurp(dir + "/" + name, file, n)) { std::printf("cannot read %s\n", name.c_str()); return 1; }
        const size_t px = (size_t)H * W;
        uint16_t *out = (uint16_t *)std::malloc(px * 2);            // exactly the plane
        std::memset(out, 0x5a, px * 2);
        const int status = decode(file, n, page, H, W, out);
        if (status != expect) { std::printf("%s page %d: status %d, expected %d\n", name.c_str(), page, status, expect); return 1; }
        if (status == TIFF_OK && !pixels.empty()) {
            uint8_t *ref = nullptr;
            size_t rn = 0;
            if (!slurp(dir + "/" + pixels, ref, rn) || rn != px * 2 || std::memcmp(ref, out, rn) != 0) {
                std::printf("%s page %d: pixels differ from the reference decode\n", name.c_str(), page);
                return 1;
            }
            std::free(ref);
        }
        if (status != TIFF_OK)
            for (size_t i = 0; i < px; i++)
                if (out[i] != 0x5a5a) { std::printf("%s: a plane that is not ok was written\n", name.c_str()); return 1; }
        by_status[status]++;
        cases++;
        if (n < 4096) {
            for (size_t cut = 0; cut < n; cut++) {                  // every truncation, in a block of exactly that size
                uint8_t *part = (uint8_t *)std::malloc(cut ? cut : 1);
                std::memcpy(part, file, cut);
                decode(part, cut, page, H, W, out);
                std::free(part);
                mutated++;
            }
            for (size_t at = 0; at < n; at++) {                     // every byte damaged three ways
                const uint8_t keep = file[at];
                for (uint8_t v : {(uint8_t)0x00, (uint8_t)0xff, (uint8_t)~keep}) {
                    file[at] = v;
                    decode(file, n, page, H, W, out);
                    mutated++;
                }
                file[at] = keep;
            }
        }
        std::free(out);
        std::free(file);
    }
    std::printf("tiff_sanitize: %zu cases (%zu ok, %zu fallback, %zu corrupt), %zu damaged variants, clean\n", cases, by_status[0], by_status[1],
                by_status[2], mutated);
    return cases ? 0 : 1;
}
