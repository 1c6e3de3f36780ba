// BC7 / BC5 / BC4 texel decode, one body for the host (bcn.cpp: vxpt_bc_decode, the expanding
// loader) and the device (vx_device.hpp: the sampler's block fetch).  A texel is decoded straight
// from its block's words; nothing is kept between texels.
//
// BC7 (the reference's 3/4-channel format, TextureManager.cu:193-198): eight modes; per mode the
// fields below, packed low bit first: mode (unary, mode + 1 bits), partition, rotation, index
// selection, the colour endpoints channel by channel (every endpoint's R, then G, then B), the alpha
// endpoints, the p-bits, the primary indices and the secondary indices.  The anchor texel of each
// subset stores its index one bit short (the high bit is 0).  A texel is
// ((64 - w) e0 + w e1 + 32) >> 6 of its subset's endpoints.  First byte 0 (the reserved mode)
// decodes to (0, 0, 0, 0), as Direct3D defines.
// BC4 / BC5 (1 / 2 channels, :199-210): per channel two 8-bit endpoints and sixteen 3-bit indices;
// the 8-value palette when e0 > e1, else 6 values and the constants 0 and 255.  The interpolants
// are 8-bit, in truncating integer division (the reference's hardware keeps more bits).
#pragma once
#include <cstdint>
#include "vx_math.hpp"
#define VX_BCN_TABLE static constexpr
#include "bcn_tables.hpp"

namespace vx {
namespace bcn {

// vxpt_bc_format (include/vxpt.h)
constexpr int kBc4 = 4, kBc5 = 5, kBc7 = 7;
VX_HD int bytes_per_block(int format) { return format == kBc4 ? 8 : 16; }

// per mode, one nibble each from bit 0: subsets, partition bits, rotation bits, index-selection bit,
// colour bits, alpha bits, per-endpoint p-bit, shared p-bit
VX_BCN_TABLE uint32_t kBc7Mode[8] = {0x01040043u, 0x10060062u, 0x00050063u, 0x01070062u,
                                     0x00651201u, 0x00870201u, 0x01770001u, 0x01550062u};
// primary index bits | secondary index bits << 4
VX_BCN_TABLE uint8_t kBc7Index[8] = {0x03, 0x03, 0x02, 0x02, 0x32, 0x22, 0x04, 0x02};
// interpolation weights of 2-, 3- and 4-bit indices at [0], [4], [12]
VX_BCN_TABLE uint8_t kBc7Weight[28] = {0, 21, 43, 64, 0, 9, 18, 27, 37, 46, 55, 64,
                                       0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};

struct Block128 {
    uint32_t w[4];
};
struct Rgba {
    int r, g, b, a;
};

// n <= 8 bits from bit pos of the block (pos + n <= 128)
VX_HD uint32_t bits(const Block128 &b, int pos, int n) {
    const int i = pos >> 5, sh = pos & 31;
    const uint32_t lo = i == 0 ? b.w[0] : i == 1 ? b.w[1] : i == 2 ? b.w[2] : b.w[3];
    const uint32_t hi = i == 0 ? b.w[1] : i == 1 ? b.w[2] : i == 2 ? b.w[3] : 0u;
    const uint64_t v = (uint64_t)lo | ((uint64_t)hi << 32);
    return (uint32_t)(v >> sh) & ((1u << n) - 1u);
}
// an endpoint value of n bits (with its p-bit already appended) widened to 8
VX_HD int widen(uint32_t v, int n) {
    v <<= 8 - n;
    return (int)(v | (v >> n));
}
VX_HD int lerp64(int e0, int e1, int w) { return ((64 - w) * e0 + w * e1 + 32) >> 6; }
VX_HD int weight(int nbits, uint32_t idx) { return kBc7Weight[(nbits == 2 ? 0 : nbits == 3 ? 4 : 12) + (int)idx]; }

// texel t = x + 4 y of a BC7 block
VX_HD Rgba bc7_texel(const Block128 &b, int t) {
    const uint32_t first = b.w[0] & 0xffu;
    if (first == 0u) return Rgba{0, 0, 0, 0};
    const int mode = __builtin_ctz(first);
    const uint32_t m = kBc7Mode[mode];
    const int ns = m & 15, pb = (m >> 4) & 15, rb = (m >> 8) & 15, isb = (m >> 12) & 15;
    const int cb = (m >> 16) & 15, ab = (m >> 20) & 15, epb = (m >> 24) & 15, spb = (m >> 28) & 15;
    const int ib = kBc7Index[mode] & 15, ib2 = kBc7Index[mode] >> 4;
    int pos = mode + 1;
    const int part = (int)bits(b, pos, pb);
    pos += pb;
    const int rot = (int)bits(b, pos, rb);
    pos += rb;
    const int sel = (int)bits(b, pos, isb);
    pos += isb;
    // the texel's subset and the subsets' anchors
    int sub = 0, anc1 = 16, anc2 = 16;  // 16: no such subset
    if (ns == 2) {
        sub = (kBc7Part2[part] >> t) & 1;
        anc1 = kBc7Anchor[part] & 15;
    } else if (ns == 3) {
        sub = (kBc7Part3[part] >> (2 * t)) & 3;
        anc1 = (kBc7Anchor[part] >> 4) & 15;
        anc2 = (kBc7Anchor[part] >> 8) & 15;
    }
    const int ne = 2 * ns, e0 = 2 * sub, e1 = e0 + 1;
    uint32_t c0[4], c1[4];
    for (int ch = 0; ch < 3; ++ch) {
        c0[ch] = bits(b, pos + (ch * ne + e0) * cb, cb);
        c1[ch] = bits(b, pos + (ch * ne + e1) * cb, cb);
    }
    pos += 3 * ne * cb;
    c0[3] = c1[3] = 0u;
    if (ab) {
        c0[3] = bits(b, pos + e0 * ab, ab);
        c1[3] = bits(b, pos + e1 * ab, ab);
        pos += ne * ab;
    }
    int cn = cb, an = ab;
    if (epb | spb) {
        const uint32_t p0 = bits(b, pos + (epb ? e0 : sub), 1), p1 = bits(b, pos + (epb ? e1 : sub), 1);
        pos += epb ? ne : ns;
        for (int ch = 0; ch < 4; ++ch) {
            c0[ch] = (c0[ch] << 1) | p0;
            c1[ch] = (c1[ch] << 1) | p1;
        }
        ++cn;
        ++an;
    }
    int q0[4], q1[4];
    for (int ch = 0; ch < 3; ++ch) {
        q0[ch] = widen(c0[ch], cn);
        q1[ch] = widen(c1[ch], cn);
    }
    q0[3] = ab ? widen(c0[3], an) : 255;
    q1[3] = ab ? widen(c1[3], an) : 255;
    // primary index: texels before t take ib bits each, less one per anchor among them
    const int anchor = sub == 0 ? 0 : sub == 1 ? anc1 : anc2;
    const int before = (t > 0) + (t > anc1) + (t > anc2);
    const uint32_t i1 = bits(b, pos + t * ib - before, ib - (t == anchor));
    int wc = weight(ib, i1), wa = wc;
    if (ib2) {
        pos += 16 * ib - 1;
        const uint32_t i2 = bits(b, pos + t * ib2 - (t > 0), ib2 - (t == 0));
        wa = weight(ib2, i2);
        if (sel) {
            const int s = wc;
            wc = wa;
            wa = s;
        }
    }
    Rgba o{lerp64(q0[0], q1[0], wc), lerp64(q0[1], q1[1], wc), lerp64(q0[2], q1[2], wc), lerp64(q0[3], q1[3], wa)};
    if (rot == 1) { const int s = o.a; o.a = o.r; o.r = s; }
    if (rot == 2) { const int s = o.a; o.a = o.g; o.g = s; }
    if (rot == 3) { const int s = o.a; o.a = o.b; o.b = s; }
    return o;
}

// texel t of one BC4 channel block (lo = bytes 0-3, hi = bytes 4-7)
VX_HD int bc4_texel(uint32_t lo, uint32_t hi, int t) {
    const int e0 = (int)(lo & 255u), e1 = (int)((lo >> 8) & 255u);
    const uint64_t v = (uint64_t)lo | ((uint64_t)hi << 32);
    const int idx = (int)((v >> (16 + 3 * t)) & 7u);
    if (idx == 0) return e0;
    if (idx == 1) return e1;
    const int k = idx - 1;
    if (e0 > e1) return ((7 - k) * e0 + k * e1) / 7;
    if (idx == 6) return 0;
    if (idx == 7) return 255;
    return ((5 - k) * e0 + k * e1) / 5;
}

// texel t of a block of the format, expanded as the loaders expand channels: BC4 -> (v, 0, 0, 255),
// BC5 -> (v, a, 0, 255).  A BC4 block is w[0], w[1].
VX_HD Rgba texel(int format, const Block128 &b, int t) {
    if (format == kBc7) return bc7_texel(b, t);
    Rgba o{bc4_texel(b.w[0], b.w[1], t), 0, 0, 255};
    if (format == kBc5) o.g = bc4_texel(b.w[2], b.w[3], t);
    return o;
}

}  // namespace bcn
}  // namespace vx
