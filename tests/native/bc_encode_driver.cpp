// CPU driver of csrc/bcn_encode.hpp (tests/test_bc_encode_search.py), built with the address and
// undefined-behaviour sanitizers: a few hundred pseudo-random and edge-case blocks through both
// qualities of every format.  Each block is decoded again and the quality-1 block must be no worse
// than the quality-0 one.
//   bc_encode_driver <out.bin>
// out.bin: the texels (n x 16 RGBA8), then the BC7, BC5, BC4 blocks at quality 0 and the same at quality 1.
// stdout: "blocks <n>"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "bcn_encode.hpp"

using namespace vx::bcn;

static uint32_t g_state = 12345u;
static uint32_t rnd() {  // xorshift32
    g_state ^= g_state << 13;
    g_state ^= g_state >> 17;
    g_state ^= g_state << 5;
    return g_state;
}

static uint32_t block_error(int format, const uint32_t *px, const Block128 &b, int nch) {
    uint32_t total = 0;
    for (int t = 0; t < 16; ++t) {
        const Rgba o = texel(format, b, t);
        const int d[4] = {enc::ch(px, t, 0) - o.r, enc::ch(px, t, 1) - o.g, enc::ch(px, t, 2) - o.b, enc::ch(px, t, 3) - o.a};
        for (int c = 0; c < nch; ++c) total += (uint32_t)(d[c] * d[c]);
    }
    return total;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<uint32_t> px;
    auto add = [&](auto f) {
        for (int t = 0; t < 16; ++t) px.push_back(f(t));
    };
    add([](int) { return 0u; });                                        // all equal
    add([](int) { return 0xffffffffu; });
    add([](int) { return 0xff4dc80du; });
    add([](int) { return 0x00123456u; });                               // alpha 0
    add([](int t) { return (t & 1) ? 0xff000000u : 0xffffffffu; });     // two values, 0 / 255 only
    add([](int t) { return (t & 5) ? 0x00000000u : 0xffffffffu; });
    add([](int t) { return (t % 3) ? 0xff102030u : 0xffc8e6fau; });     // two values
    add([](int t) { return (t < 8) ? 0x80010203u : 0x7ffefdfcu; });
    add([](int t) { return (uint32_t)t * 0x11111111u; });               // a grey ramp with alpha
    add([](int t) { return 0xff000000u | (uint32_t)(t * 17) | ((uint32_t)(255 - t * 17) << 8); });
    add([](int t) { return t == 5 ? 0x00ffffffu : 0xffffffffu; });      // one transparent texel
    for (int k = 0; k < 120; ++k) add([](int) { return rnd(); });                        // noise, random alpha
    for (int k = 0; k < 120; ++k) add([](int) { return rnd() | 0xff000000u; });          // opaque noise
    for (int k = 0; k < 60; ++k) {                                                       // two noisy colour clusters
        const uint32_t a = rnd(), b = rnd(), m = rnd();
        add([&](int t) { return ((((m >> t) & 1u) ? a : b) ^ (rnd() & 0x03030303u)) | 0xff000000u; });
    }
    for (int k = 0; k < 40; ++k) {                                                       // few levels incl. 0 and 255
        const uint32_t base = rnd() & 0x7f7f7f7fu;
        add([&](int) {
            const uint32_t r = rnd() % 6u;
            return r == 0 ? 0u : r == 1 ? 0xffffffffu : base + (r - 2) * 0x02020202u;
        });
    }
    const int n = (int)(px.size() / 16);
    std::vector<uint8_t> out[2][3];
    long bad = 0;
    for (int q = 0; q < 2; ++q)
        for (int i = 0; i < n; ++i) {
            const uint32_t *p = px.data() + 16 * i;
            Block128 b7{}, b5{};
            enc::encode_bc7_host(p, q, b7.w);
            const uint64_t r = enc::encode_bc4(p, 0, q), g = enc::encode_bc4(p, 1, q);
            b5.w[0] = (uint32_t)r;
            b5.w[1] = (uint32_t)(r >> 32);
            b5.w[2] = (uint32_t)g;
            b5.w[3] = (uint32_t)(g >> 32);
            const uint8_t *s7 = reinterpret_cast<const uint8_t *>(b7.w), *s5 = reinterpret_cast<const uint8_t *>(b5.w);
            out[q][0].insert(out[q][0].end(), s7, s7 + 16);
            out[q][1].insert(out[q][1].end(), s5, s5 + 16);
            out[q][2].insert(out[q][2].end(), s5, s5 + 8);
            if ((b7.w[0] & 255u) == 0u && bad++ < 5) std::printf("block %d quality %d: first byte 0\n", i, q);
            if (q == 1) {
                Block128 f7{}, f5{};
                std::memcpy(f7.w, out[0][0].data() + 16 * (size_t)i, 16);
                std::memcpy(f5.w, out[0][1].data() + 16 * (size_t)i, 16);
                if (block_error(kBc7, p, b7, 4) > block_error(kBc7, p, f7, 4) && bad++ < 5) std::printf("block %d: BC7 worse\n", i);
                if (block_error(kBc5, p, b5, 2) > block_error(kBc5, p, f5, 2) && bad++ < 5) std::printf("block %d: BC5 worse\n", i);
                if (block_error(kBc4, p, b5, 1) > block_error(kBc4, p, f5, 1) && bad++ < 5) std::printf("block %d: BC4 worse\n", i);
            }
        }
    std::ofstream o(argv[1], std::ios::binary);
    o.write(reinterpret_cast<const char *>(px.data()), (std::streamsize)(px.size() * 4));
    for (int q = 0; q < 2; ++q)
        for (int f = 0; f < 3; ++f) o.write(reinterpret_cast<const char *>(out[q][f].data()), (std::streamsize)out[q][f].size());
    std::printf("blocks %d\n", n);
    return bad ? 1 : 0;
}
