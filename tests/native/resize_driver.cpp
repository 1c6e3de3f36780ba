// CPU driver of csrc/resize.hpp (tests/test_resize.py), built with the address and undefined-behaviour
// sanitizers: every pixel size through shape pairs that shrink, grow, keep and degenerate to one pixel,
// on heap buffers of exactly the planes' sizes, so that a read or a store one element out of a plane is
// reported.  Each result is checked against the map written out with 64-bit arithmetic.
//   resize_driver <out.bin>
// out.bin: the 20-byte-pixel resample of the 50 x 37 counting pattern to 33 x 21 (compared with the
// library's by the test).  stdout: "cases <n>"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "resize.hpp"

using namespace vx::resize;

static int check(int ow, int oh, int nw, int nh, int bpp, std::vector<uint8_t> *keep) {
    std::vector<uint8_t> src((size_t)ow * oh * bpp), dst((size_t)nw * nh * bpp, 0xEE);
    for (size_t i = 0; i < src.size() / 4; ++i) {
        const uint32_t v = (uint32_t)i * 7u;
        std::memcpy(&src[4 * i], &v, 4);
    }
    resize_host(src.data(), dst.data(), Map{ow, oh, nw, nh}, bpp);
    for (int y = 0; y < nh; ++y)
        for (int x = 0; x < nw; ++x) {
            long long sx = ((2LL * x + 1) * ow) / (2LL * nw), sy = ((2LL * y + 1) * oh) / (2LL * nh);
            if (sx > ow - 1) sx = ow - 1;
            if (sy > oh - 1) sy = oh - 1;
            if (std::memcmp(&dst[((size_t)y * nw + x) * bpp], &src[((size_t)sy * ow + sx) * bpp], bpp) != 0) {
                std::fprintf(stderr, "%dx%d -> %dx%d, %d bytes: pixel (%d, %d) is not (%lld, %lld)\n", ow, oh, nw, nh, bpp,
                             x, y, sx, sy);
                return 1;
            }
        }
    if (keep) *keep = dst;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const int shapes[][4] = {{96, 64, 64, 48}, {64, 48, 96, 64}, {50, 37, 33, 21}, {33, 21, 50, 37}, {7, 5, 7, 5},
                             {1, 1, 5, 3},     {5, 3, 1, 1},     {3, 2, 301, 2},   {301, 2, 3, 1},   {1, 9, 1, 4}};
    int cases = 0;
    std::vector<uint8_t> keep;
    for (const auto &s : shapes)
        for (int bpp : {4, 16, 20, 32}) {
            const bool kept = s[0] == 50 && bpp == 20;
            if (check(s[0], s[1], s[2], s[3], bpp, kept ? &keep : nullptr)) return 1;
            ++cases;
        }
    // the largest sizes the map takes: (2x + 1) * old must stay inside 32 bits
    if (src_index(kResizeMaxDim - 1, kResizeMaxDim, kResizeMaxDim) != kResizeMaxDim - 1 ||
        src_index(kResizeMaxDim - 1, kResizeMaxDim, 1 + (kResizeMaxDim - 1)) != kResizeMaxDim - 1 ||
        src_index(0, kResizeMaxDim, 1) != kResizeMaxDim / 2 || src_index(kResizeMaxDim - 1, 1, kResizeMaxDim) != 0)
        return 1;
    std::ofstream(argv[1], std::ios::binary).write((const char *)keep.data(), (std::streamsize)keep.size());
    std::printf("cases %d\n", cases);
    return 0;
}
