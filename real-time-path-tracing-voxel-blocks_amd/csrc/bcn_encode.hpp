// BC7 / BC5 / BC4 block encoders, one set of bodies for the host (bcn.cpp: vxpt_bc_encode,
// vxpt_bc_encode_q, the loaders) and the device (bcn_encode.hip).  Every selection is made on
// integers, and the fits are integer too (no float anywhere), so host and device emit the same bytes.
//
// A block's 16 texels are 16 packed words (r | g << 8 | b << 16 | a << 24, texel t = x + 4 y) behind
// one pointer: a stack array on the host, a wave-uniform LDS row on the device.
//
// Quality 0 is the fast encoder (encode_bc7_fast, encode_bc4_fast): BC7 mode 6 on the diagonal of
// the block's colour box, BC4 max / min endpoints in the 8-value mode.
// Quality 1 is a search.  Every candidate has an ordinal and an error, the sum over the block of the
// squared channel differences against the palette the decoder builds (lerp64, widen, kBc7Weight of
// bcn_decode.hpp); the smallest (error, ordinal) pair wins, so a tie goes to the lower ordinal.
//   BC7 ordinal 0          the quality-0 block, its error measured through bc7_texel
//       1-4                mode 6, endpoints from the principal-axis fit, p-bits (p0, p1) = (0,0) (1,0) (0,1) (1,1)
//       5-8                mode 6, one least-squares refinement on the indices of the best of 1-4, same p-bits
//       9                  mode 5, rotation 0 (blocks with an alpha other than 255)
//       16 + p, 80 + p     modes 1 and 3 with partition p (blocks whose alpha is 255 throughout)
//       144 + p            mode 7 with partition p (the other blocks)
//   BC4 ordinal 0          the quality-0 block
//       1 + 4 a + b        8-value mode, e0 = max - a, e1 = min + b, a and b in [0, kBc4Inset]
//       17 + 4 a + b       6-value mode (blocks holding 0 or 255), e0 = lo + a, e1 = hi - b over the other values
// The partitioned candidates are one call per partition (bc7_partition_candidates): lane p of a
// wavefront on the device, a loop on the host.
#pragma once
#include "bcn_decode.hpp"

namespace vx {
namespace bcn {
namespace enc {

// inset window of the BC4 endpoint search: levels tried inward from each extreme
constexpr int kBc4Inset = 3;
constexpr int kOrdMode6 = 1, kOrdMode6Refined = 5, kOrdMode5 = 9, kOrdMode1 = 16, kOrdMode3 = 80, kOrdMode7 = 144;
constexpr int kOrdBc4Eight = 1, kOrdBc4Six = 17;

VX_HD int ch(const uint32_t *px, int t, int c) { return (int)((px[t] >> (8 * c)) & 255u); }

// ------------------------------------------------------------------ quality 0 (the fast encoder)

// 16 values -> one BC4 channel block: endpoints max, min in the 8-value mode (e0 > e1), nearest
// palette entry per texel (ties: the lower index); a constant block is e0 = e1 with index 0
VX_HD uint64_t encode_bc4_fast(const uint32_t *px, int c) {
    int mx = ch(px, 0, c), mn = mx;
    for (int t = 1; t < 16; ++t) {
        const int v = ch(px, t, c);
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
    uint64_t bitsOut = (uint64_t)mx | ((uint64_t)mn << 8);
    if (mx > mn) {
        int pal[8] = {mx, mn};
        for (int k = 1; k <= 6; ++k) pal[k + 1] = ((7 - k) * mx + k * mn) / 7;
        for (int t = 0; t < 16; ++t) {
            const int v = ch(px, t, c);
            int best = 0, bestErr = 1 << 30;
            for (int i = 0; i < 8; ++i) {
                const int e = v > pal[i] ? v - pal[i] : pal[i] - v;
                if (e < bestErr) {
                    bestErr = e;
                    best = i;
                }
            }
            bitsOut |= (uint64_t)best << (16 + 3 * t);
        }
    }
    return bitsOut;
}

// fields appended low bit first
struct Bits128 {
    uint64_t lo = 0, hi = 0;
    int pos = 0;
    VX_HD void put(uint32_t v, int n) {  // n <= 8 bits of v at pos
        if (pos < 64) {
            lo |= (uint64_t)v << pos;
            if (pos + n > 64) hi |= (uint64_t)v >> (64 - pos);
        } else {
            hi |= (uint64_t)v << (pos - 64);
        }
        pos += n;
    }
    VX_HD void store(uint32_t out[4]) const {
        out[0] = (uint32_t)lo;
        out[1] = (uint32_t)(lo >> 32);
        out[2] = (uint32_t)hi;
        out[3] = (uint32_t)(hi >> 32);
    }
};

// a mode-6 endpoint is 8 bits per channel whose low bit is the endpoint's one p-bit: the value
// with low bit p nearest to num / den (ties: the lower)
VX_HD int nearest_with_lsb(int num, int den, int p) {
    int best = p, bestErr = 1 << 30;
    const int x = num / den, first = x < 4 ? p : (((x - 3) & ~1) | p);
    for (int e = first; e < 256 && e <= x + 3; e += 2) {
        const int d = e * den - num, err = d < 0 ? -d : d;
        if (err < bestErr) {
            bestErr = err;
            best = e;
        }
    }
    return best;
}
// the p-bit (0 on a tie) and channel values for targets num[c] / den that leave the smaller summed distance
VX_HD void quantise_endpoint(const int num[4], int den, int e[4]) {
    int bestSum = 1 << 30;
    for (int p = 0; p < 2; ++p) {
        int q[4], sum = 0;
        for (int c = 0; c < 4; ++c) {
            q[c] = nearest_with_lsb(num[c], den, p);
            const int d = q[c] * den - num[c];
            sum += d < 0 ? -d : d;
        }
        if (sum < bestSum) {
            bestSum = sum;
            for (int c = 0; c < 4; ++c) e[c] = q[c];
        }
    }
}
// indices of the 16 texels on the palette of e0, e1 (nearest in summed squared error, ties: the lower
// index), four bits per texel from bit 4 t; returns the block's largest absolute channel error
VX_HD int fit_indices(const uint32_t *px, const int e0[4], const int e1[4], uint64_t &idx) {
    int pal[16][4];
    for (int i = 0; i < 16; ++i)
        for (int c = 0; c < 4; ++c) pal[i][c] = lerp64(e0[c], e1[c], kBc7Weight[12 + i]);
    int worst = 0;
    idx = 0;
    for (int t = 0; t < 16; ++t) {
        int best = 0, bestErr = 1 << 30;
        int bp[4] = {0, 0, 0, 0};
        const int x[4] = {ch(px, t, 0), ch(px, t, 1), ch(px, t, 2), ch(px, t, 3)};
        for (int i = 0; i < 16; ++i) {
            int err = 0;
            for (int c = 0; c < 4; ++c) err += (x[c] - pal[i][c]) * (x[c] - pal[i][c]);
            if (err < bestErr) {
                bestErr = err;
                best = i;
                for (int c = 0; c < 4; ++c) bp[c] = pal[i][c];
            }
        }
        idx |= (uint64_t)best << (4 * t);
        for (int c = 0; c < 4; ++c) {
            const int d = x[c] - bp[c];
            worst = (d < 0 ? -d : d) > worst ? (d < 0 ? -d : d) : worst;
        }
    }
    return worst;
}

// a mode-6 block of endpoints e0, e1 (8-bit values, low bit = p-bit) and 4-bit indices; the anchor's
// index keeps its high bit 0: the endpoints are swapped otherwise
VX_HD void pack_mode6(const int a[4], const int b[4], uint64_t idx, uint32_t out[4]) {
    const bool swap = ((idx >> 3) & 1u) != 0;
    if (swap) idx = ~idx;
    Bits128 w;
    w.put(1u << 6, 7);
    for (int c = 0; c < 4; ++c) {
        w.put((uint32_t)(swap ? b[c] : a[c]) >> 1, 7);
        w.put((uint32_t)(swap ? a[c] : b[c]) >> 1, 7);
    }
    w.put((uint32_t)(swap ? b[0] : a[0]) & 1u, 1);
    w.put((uint32_t)(swap ? a[0] : b[0]) & 1u, 1);
    w.put((uint32_t)idx & 7u, 3);
    for (int t = 1; t < 16; ++t) w.put((uint32_t)(idx >> (4 * t)) & 15u, 4);
    w.store(out);
}

// 16 RGBA texels -> a BC7 mode-6 block.  Endpoints: the corners of the block's colour box along its
// diagonal, each channel's direction taken from the sign of its covariance with the widest channel;
// kept unless the block's mean colour as both endpoints has the smaller largest error.
VX_HD void encode_bc7_fast(const uint32_t *px, uint32_t out[4]) {
    int mn[4], mx[4], sum[4];
    for (int c = 0; c < 4; ++c) {
        mn[c] = mx[c] = sum[c] = ch(px, 0, c);
        for (int t = 1; t < 16; ++t) {
            const int v = ch(px, t, c);
            mn[c] = v < mn[c] ? v : mn[c];
            mx[c] = v > mx[c] ? v : mx[c];
            sum[c] += v;
        }
    }
    int ref = 0, refW = mx[0] - mn[0], refSum = sum[0];
    for (int c = 1; c < 4; ++c)
        if (mx[c] - mn[c] > refW) {
            ref = c;
            refW = mx[c] - mn[c];
            refSum = sum[c];
        }
    int lo[4], hi[4];
    for (int c = 0; c < 4; ++c) {
        long long cov = 0;  // 256 x the covariance with the widest channel
        for (int t = 0; t < 16; ++t)
            cov += (long long)(16 * ch(px, t, c) - sum[c]) * (16 * (int)((px[t] >> (8 * ref)) & 255u) - refSum);
        lo[c] = cov < 0 ? mx[c] : mn[c];
        hi[c] = cov < 0 ? mn[c] : mx[c];
    }
    int e0[4], e1[4], m[4];
    uint64_t idx, midx;
    quantise_endpoint(lo, 1, e0);
    quantise_endpoint(hi, 1, e1);
    const int worst = fit_indices(px, e0, e1, idx);
    quantise_endpoint(sum, 16, m);
    if (fit_indices(px, m, m, midx) < worst) {
        for (int c = 0; c < 4; ++c) e0[c] = e1[c] = m[c];
        idx = midx;
    }
    pack_mode6(e0, e1, idx, out);
}

// ------------------------------------------------------------------ quality 1 (the search)

// the running winner of a block (or of a lane's share of it): smallest (err, ord)
struct Best {
    uint32_t err = 0xffffffffu, ord = 0xffffffffu;
    uint32_t w[4] = {0, 0, 0, 0};
    VX_HD bool beats(uint32_t e, uint32_t o) const { return e < err || (e == err && o < ord); }
    VX_HD uint64_t key() const { return ((uint64_t)err << 32) | ord; }
};

// an 8-bit target -> the n-bit code (its low bit fixed to p when p >= 0) whose widened value is nearest
// (ties: the lower code)
VX_HD int quantise(int target, int n, int p) {
    const int step = p >= 0 ? 2 : 1;
    int c = target >> (8 - n);
    if (p >= 0) c = (c & ~1) | p;
    int best = c, bestD = 1 << 30;
    for (int k = -1; k <= 1; ++k) {
        const int q = c + k * step;
        if (q < 0 || q >= (1 << n)) continue;
        const int d = widen((uint32_t)q, n) - target, ad = d < 0 ? -d : d;
        if (ad < bestD) {
            bestD = ad;
            best = q;
        }
    }
    return best;
}
// NC channels of one endpoint with one p-bit of its own: the p (0 on a tie) with the smaller summed
// squared distance.  code[c] = the n-bit codes, val[c] = their 8-bit values
template <int NC>
VX_HD void quantise_own_p(const int target[4], int n, int code[4], int val[4]) {
    int bestSum = 1 << 30;
    for (int p = 0; p < 2; ++p) {
        int q[NC], sum = 0;
        for (int c = 0; c < NC; ++c) {
            q[c] = quantise(target[c], n, p);
            const int d = widen((uint32_t)q[c], n) - target[c];
            sum += d * d;
        }
        if (sum < bestSum) {
            bestSum = sum;
            for (int c = 0; c < NC; ++c) {
                code[c] = q[c];
                val[c] = widen((uint32_t)q[c], n);
            }
        }
    }
}

VX_HD long long rdiv(long long num, long long den) {  // num / den to nearest, den > 0; negative -> 0
    return num <= 0 ? 0 : (2 * num + den) / (2 * den);
}
VX_HD int to_byte(long long v) { return v < 0 ? 0 : v > 255 ? 255 : (int)v; }

// Principal-axis fit of the texels whose mask bit equals sel, over channels 0..NC-1: lo / hi = the
// subset's mean moved along the axis to its smallest / largest projection, rounded to 8 bits.  The
// axis is three power iterations on the integer covariance from its row of the largest diagonal,
// renormalised by shifts to below 2^10 (64-bit integers: no rounding that could differ between machines).
template <int NC>
VX_HD void axis_fit(const uint32_t *px, uint32_t mask, uint32_t sel, int lo[4], int hi[4]) {
    int n = 0, S[NC], M[NC][NC];
    for (int c = 0; c < NC; ++c) {
        S[c] = 0;
        for (int d = 0; d < NC; ++d) M[c][d] = 0;
    }
    for (int t = 0; t < 16; ++t) {
        const int in = ((mask >> t) & 1u) == sel ? 1 : 0;
        n += in;
        for (int c = 0; c < NC; ++c) {
            const int x = in ? ch(px, t, c) : 0;
            S[c] += x;
            for (int d = c; d < NC; ++d) M[c][d] += x * ch(px, t, d);
        }
    }
    for (int c = NC; c < 4; ++c) lo[c] = hi[c] = 255;
    long long cov[NC][NC];
    for (int c = 0; c < NC; ++c)
        for (int d = c; d < NC; ++d) cov[c][d] = cov[d][c] = (long long)n * M[c][d] - (long long)S[c] * S[d];
    long long v[NC], top = 0;
    for (int c = 0; c < NC; ++c) v[c] = 0;
    for (int r = 0; r < NC; ++r)
        if (cov[r][r] > top) {
            top = cov[r][r];
            for (int c = 0; c < NC; ++c) v[c] = cov[r][c];
        }
    // top == 0: one colour (or no texel): v stays 0 and both ends are the mean
    for (int it = 0; it < 4; ++it) {
        long long m = 0;
        for (int c = 0; c < NC; ++c) m = (v[c] < 0 ? -v[c] : v[c]) > m ? (v[c] < 0 ? -v[c] : v[c]) : m;
        const int sh = m == 0 ? 0 : 64 - __builtin_clzll((unsigned long long)m) - 10;
        if (sh > 0)
            for (int c = 0; c < NC; ++c) v[c] = v[c] >= 0 ? v[c] >> sh : -((-v[c]) >> sh);
        if (it == 3) break;
        long long u[NC];
        for (int c = 0; c < NC; ++c) {
            u[c] = 0;
            for (int d = 0; d < NC; ++d) u[c] += cov[c][d] * v[d];
        }
        for (int c = 0; c < NC; ++c) v[c] = u[c];
    }
    long long vv = 0;
    for (int c = 0; c < NC; ++c) vv += v[c] * v[c];
    int tmin = 0x7fffffff, tmax = -0x7fffffff;
    for (int t = 0; t < 16; ++t) {
        int p = 0;
        for (int c = 0; c < NC; ++c) p += (int)v[c] * (n * ch(px, t, c) - S[c]);
        const bool in = ((mask >> t) & 1u) == sel;
        tmin = in && p < tmin ? p : tmin;
        tmax = in && p > tmax ? p : tmax;
    }
    const bool flat = vv == 0 || n == 0;  // the axis is 0: the mean alone
    const long long scale = flat ? 1 : vv, den = (n == 0 ? 1 : n) * scale;
    for (int c = 0; c < NC; ++c) {
        lo[c] = to_byte(rdiv((long long)S[c] * scale + (flat ? 0 : v[c] * tmin), den));
        hi[c] = to_byte(rdiv((long long)S[c] * scale + (flat ? 0 : v[c] * tmax), den));
    }
}

// Nearest palette entry (IB index bits; ties: the lower index) for every texel over channels
// C0..C0+NC-1, the palette of a texel being that of its subset (mask bit): ep[subset][end][channel]
// 8-bit endpoint values.  Indices: four bits per texel from bit 4 t.  Returns the summed squared error.
template <int IB, int C0, int NC>
VX_HD uint32_t assign(const uint32_t *px, uint32_t mask, const int ep[2][2][4], uint64_t &idx) {
    constexpr int W0 = IB == 2 ? 0 : IB == 3 ? 4 : 12;
    uint32_t total = 0;
    idx = 0;
    for (int t = 0; t < 16; ++t) {
        const bool s = ((mask >> t) & 1u) != 0;
        int a[NC], b[NC], x[NC];
        for (int c = 0; c < NC; ++c) {
            a[c] = s ? ep[1][0][C0 + c] : ep[0][0][C0 + c];
            b[c] = s ? ep[1][1][C0 + c] : ep[0][1][C0 + c];
            x[c] = ch(px, t, C0 + c);
        }
        int best = 0, bestErr = 1 << 30;
        for (int i = 0; i < (1 << IB); ++i) {
            int err = 0;
            for (int c = 0; c < NC; ++c) {
                const int d = x[c] - lerp64(a[c], b[c], kBc7Weight[W0 + i]);
                err += d * d;
            }
            if (err < bestErr) {
                bestErr = err;
                best = i;
            }
        }
        idx |= (uint64_t)best << (4 * t);
        total += (uint32_t)bestErr;
    }
    return total;
}

// A block of the mode from codes[subset][end][channel] (with the p-bit as the low bit where the mode
// has one), primary indices idx and, in mode 5, alpha indices idx2 (four bits per texel).  Every
// subset's anchor index keeps its high bit 0: that subset's endpoints are swapped and its indices
// complemented otherwise -- in mode 5 for the colour and the alpha index sets separately.
VX_HD void pack_bc7(int mode, int part, const int code[2][2][4], uint64_t idx, uint64_t idx2, uint32_t out[4]) {
    const uint32_t m = kBc7Mode[mode];
    const int ns = m & 15, pb = (m >> 4) & 15, rb = (m >> 8) & 15, isb = (m >> 12) & 15;
    const int cb = (m >> 16) & 15, ab = (m >> 20) & 15, epb = (m >> 24) & 15, spb = (m >> 28) & 15;
    const int ib = kBc7Index[mode] & 15, ib2 = kBc7Index[mode] >> 4;
    const uint32_t mask = ns == 2 ? kBc7Part2[part] : 0u;
    const int anc1 = ns == 2 ? (kBc7Anchor[part] & 15) : 16;
    const uint32_t top = 1u << (ib - 1), full = (1u << ib) - 1u;
    const bool sw0 = (((uint32_t)idx & 15u) & top) != 0;
    const bool sw1 = ns == 2 && (((uint32_t)(idx >> (4 * (anc1 & 15))) & 15u) & top) != 0;
    const bool swA = ib2 ? (((uint32_t)idx2 & 15u) & (1u << (ib2 - 1))) != 0 : sw0;  // mode 5's alpha set
    const int pbit = (epb | spb) ? 1 : 0;
    Bits128 w;
    w.put(1u << mode, mode + 1);
    w.put((uint32_t)part, pb);
    w.put(0u, rb);
    w.put(0u, isb);
    for (int c = 0; c < 3; ++c) {
        w.put((uint32_t)(sw0 ? code[0][1][c] : code[0][0][c]) >> pbit, cb);
        w.put((uint32_t)(sw0 ? code[0][0][c] : code[0][1][c]) >> pbit, cb);
        if (ns == 2) {
            w.put((uint32_t)(sw1 ? code[1][1][c] : code[1][0][c]) >> pbit, cb);
            w.put((uint32_t)(sw1 ? code[1][0][c] : code[1][1][c]) >> pbit, cb);
        }
    }
    if (ab) {
        w.put((uint32_t)(swA ? code[0][1][3] : code[0][0][3]) >> pbit, ab);
        w.put((uint32_t)(swA ? code[0][0][3] : code[0][1][3]) >> pbit, ab);
        if (ns == 2) {
            w.put((uint32_t)(sw1 ? code[1][1][3] : code[1][0][3]) >> pbit, ab);
            w.put((uint32_t)(sw1 ? code[1][0][3] : code[1][1][3]) >> pbit, ab);
        }
    }
    if (epb) {
        w.put((uint32_t)(sw0 ? code[0][1][0] : code[0][0][0]) & 1u, 1);
        w.put((uint32_t)(sw0 ? code[0][0][0] : code[0][1][0]) & 1u, 1);
        if (ns == 2) {
            w.put((uint32_t)(sw1 ? code[1][1][0] : code[1][0][0]) & 1u, 1);
            w.put((uint32_t)(sw1 ? code[1][0][0] : code[1][1][0]) & 1u, 1);
        }
    } else if (spb) {
        w.put((uint32_t)code[0][0][0] & 1u, 1);
        if (ns == 2) w.put((uint32_t)code[1][0][0] & 1u, 1);
    }
    for (int t = 0; t < 16; ++t) {
        const bool s = ((mask >> t) & 1u) != 0;
        uint32_t i = (uint32_t)(idx >> (4 * t)) & 15u;
        if (s ? sw1 : sw0) i = full - i;
        w.put(i, ib - ((t == 0 || t == anc1) ? 1 : 0));
    }
    if (ib2) {
        const uint32_t full2 = (1u << ib2) - 1u;
        for (int t = 0; t < 16; ++t) {
            uint32_t i = (uint32_t)(idx2 >> (4 * t)) & 15u;
            if (swA) i = full2 - i;
            w.put(i, ib2 - (t == 0 ? 1 : 0));
        }
    }
    w.store(out);
}

// the summed squared error of a finished BC7 block, through the decoder
VX_HD uint32_t bc7_block_error(const uint32_t *px, const uint32_t w[4]) {
    Block128 b;
    for (int i = 0; i < 4; ++i) b.w[i] = w[i];
    uint32_t total = 0;
    for (int t = 0; t < 16; ++t) {
        const Rgba o = bc7_texel(b, t);
        const int dr = ch(px, t, 0) - o.r, dg = ch(px, t, 1) - o.g, db = ch(px, t, 2) - o.b, da = ch(px, t, 3) - o.a;
        total += (uint32_t)(dr * dr + dg * dg + db * db + da * da);
    }
    return total;
}

VX_HD bool block_opaque(const uint32_t *px) {
    uint32_t all = 0xff000000u;
    for (int t = 0; t < 16; ++t) all &= px[t];
    return (all >> 24) == 255u;
}

// mode 6 with 8-bit targets lo / hi: the four p-bit pairs from ordinal ord0.  Returns the smallest
// error among them and its indices
VX_HD uint32_t mode6_candidates(const uint32_t *px, const int lo[4], const int hi[4], uint32_t ord0, Best &best,
                                uint64_t &idxOut) {
    uint32_t bestErr = 0xffffffffu;
    for (int pc = 0; pc < 4; ++pc) {
        int ep[2][2][4];
        for (int c = 0; c < 4; ++c) {
            ep[0][0][c] = quantise(lo[c], 8, pc & 1);
            ep[0][1][c] = quantise(hi[c], 8, pc >> 1);
            ep[1][0][c] = ep[1][1][c] = 0;
        }
        uint64_t idx;
        const uint32_t err = assign<4, 0, 4>(px, 0u, ep, idx);
        if (err < bestErr) {
            bestErr = err;
            idxOut = idx;
        }
        if (best.beats(err, ord0 + pc)) {
            best.err = err;
            best.ord = ord0 + pc;
            pack_mode6(ep[0][0], ep[0][1], idx, best.w);
        }
    }
    return bestErr;
}

// the candidates that have no partition: the quality-0 block, mode 6 fitted and refined, mode 5
VX_HD void bc7_shared_candidates(const uint32_t *px, bool opaque, Best &best) {
    uint32_t q0[4];
    encode_bc7_fast(px, q0);
    const uint32_t e0 = bc7_block_error(px, q0);
    if (best.beats(e0, 0u)) {
        best.err = e0;
        best.ord = 0u;
        for (int i = 0; i < 4; ++i) best.w[i] = q0[i];
    }
    int lo[4], hi[4];
    axis_fit<4>(px, 0u, 0u, lo, hi);
    uint64_t idx = 0;
    mode6_candidates(px, lo, hi, kOrdMode6, best, idx);
    // least squares on the chosen indices: minimise sum (64 x - (64 - w) a - w b)^2 per channel
    long long A = 0, B = 0, C = 0, P[4] = {0, 0, 0, 0}, Q[4] = {0, 0, 0, 0};
    for (int t = 0; t < 16; ++t) {
        const int wt = kBc7Weight[12 + (int)((idx >> (4 * t)) & 15u)], wn = 64 - wt;
        A += wn * wn;
        B += wn * wt;
        C += wt * wt;
        for (int c = 0; c < 4; ++c) {
            P[c] += wn * ch(px, t, c);
            Q[c] += wt * ch(px, t, c);
        }
    }
    const long long det = A * C - B * B;
    if (det > 0) {
        int rlo[4], rhi[4];
        for (int c = 0; c < 4; ++c) {
            rlo[c] = to_byte(rdiv(64 * (C * P[c] - B * Q[c]), det));
            rhi[c] = to_byte(rdiv(64 * (A * Q[c] - B * P[c]), det));
        }
        uint64_t ridx;
        mode6_candidates(px, rlo, rhi, kOrdMode6Refined, best, ridx);
    }
    if (!opaque) {  // mode 5: 7-bit colour and 8-bit alpha endpoints, each with 2-bit indices of its own
        int clo[4], chi[4], code[2][2][4], ep[2][2][4];
        axis_fit<3>(px, 0u, 0u, clo, chi);
        int amn = 255, amx = 0;
        for (int t = 0; t < 16; ++t) {
            const int a = ch(px, t, 3);
            amn = a < amn ? a : amn;
            amx = a > amx ? a : amx;
        }
        for (int c = 0; c < 3; ++c) {
            code[0][0][c] = quantise(clo[c], 7, -1);
            code[0][1][c] = quantise(chi[c], 7, -1);
            ep[0][0][c] = widen((uint32_t)code[0][0][c], 7);
            ep[0][1][c] = widen((uint32_t)code[0][1][c], 7);
        }
        code[0][0][3] = ep[0][0][3] = amn;
        code[0][1][3] = ep[0][1][3] = amx;
        for (int c = 0; c < 4; ++c) code[1][0][c] = code[1][1][c] = ep[1][0][c] = ep[1][1][c] = 0;
        uint64_t ic, ia;
        const uint32_t err = assign<2, 0, 3>(px, 0u, ep, ic) + assign<2, 3, 1>(px, 0u, ep, ia);
        if (best.beats(err, kOrdMode5)) {
            best.err = err;
            best.ord = kOrdMode5;
            pack_bc7(5, 0, code, ic, ia, best.w);
        }
    }
}

// one partitioned mode on fitted 8-bit targets t[subset][end][channel]: NC channels of N-bit codes
// (p-bit included), OWNP: a p-bit per endpoint, else one per subset; IB index bits
template <int MODE, int NC, int N, bool OWNP, int IB>
VX_HD void partition_mode(const uint32_t *px, int part, uint32_t mask, const int tg[2][2][4], uint32_t ord, Best &best) {
    int code[2][2][4], ep[2][2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        for (int e = 0; e < 2; ++e)
            for (int c = 0; c < 4; ++c) {
                code[s][e][c] = 0;
                ep[s][e][c] = 255;
            }
        if (OWNP) {
            quantise_own_p<NC>(tg[s][0], N, code[s][0], ep[s][0]);
            quantise_own_p<NC>(tg[s][1], N, code[s][1], ep[s][1]);
        } else {  // the subset's two endpoints share the p-bit: 0 on a tie
            int bestSum = 1 << 30;
            for (int p = 0; p < 2; ++p) {
                int q[2][NC], sum = 0;
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        q[e][c] = quantise(tg[s][e][c], N, p);
                        const int d = widen((uint32_t)q[e][c], N) - tg[s][e][c];
                        sum += d * d;
                    }
                if (sum < bestSum) {
                    bestSum = sum;
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            code[s][e][c] = q[e][c];
                            ep[s][e][c] = widen((uint32_t)q[e][c], N);
                        }
                }
            }
        }
    }
    uint64_t idx;
    const uint32_t err = assign<IB, 0, NC>(px, mask, ep, idx);
    if (best.beats(err, ord)) {
        best.err = err;
        best.ord = ord;
        pack_bc7(MODE, part, code, idx, 0, best.w);
    }
}

// the candidates of two-subset partition part (0..63): modes 1 and 3 for an opaque block, mode 7 otherwise
VX_HD void bc7_partition_candidates(const uint32_t *px, int part, bool opaque, Best &best) {
    const uint32_t mask = kBc7Part2[part];
    int tg[2][2][4];
    if (opaque) {
        axis_fit<3>(px, mask, 0u, tg[0][0], tg[0][1]);
        axis_fit<3>(px, mask, 1u, tg[1][0], tg[1][1]);
        partition_mode<1, 3, 7, false, 3>(px, part, mask, tg, (uint32_t)(kOrdMode1 + part), best);
        partition_mode<3, 3, 8, true, 2>(px, part, mask, tg, (uint32_t)(kOrdMode3 + part), best);
    } else {
        axis_fit<4>(px, mask, 0u, tg[0][0], tg[0][1]);
        axis_fit<4>(px, mask, 1u, tg[1][0], tg[1][1]);
        partition_mode<7, 4, 6, true, 2>(px, part, mask, tg, (uint32_t)(kOrdMode7 + part), best);
    }
}

// ------------------------------------------------------------------ BC4 search

// indices and summed squared error of channel c on the decoder's palette of (e0, e1)
VX_HD uint32_t bc4_assign(const uint32_t *px, int c, int e0, int e1, uint64_t &bitsOut) {
    int pal[8] = {e0, e1, 0, 0, 0, 0, 0, 0};
    if (e0 > e1) {
        for (int k = 1; k <= 6; ++k) pal[k + 1] = ((7 - k) * e0 + k * e1) / 7;
    } else {
        for (int k = 1; k <= 4; ++k) pal[k + 1] = ((5 - k) * e0 + k * e1) / 5;
        pal[6] = 0;
        pal[7] = 255;
    }
    uint32_t total = 0;
    bitsOut = (uint64_t)e0 | ((uint64_t)e1 << 8);
    for (int t = 0; t < 16; ++t) {
        const int v = ch(px, t, c);
        int best = 0, bestErr = 1 << 30;
        for (int i = 0; i < 8; ++i) {
            const int d = v - pal[i];
            if (d * d < bestErr) {
                bestErr = d * d;
                best = i;
            }
        }
        bitsOut |= (uint64_t)best << (16 + 3 * t);
        total += (uint32_t)bestErr;
    }
    return total;
}

// one BC4 channel block of channel c at the quality
VX_HD uint64_t encode_bc4(const uint32_t *px, int c, int quality) {
    const uint64_t fast = encode_bc4_fast(px, c);
    if (quality == 0) return fast;
    uint64_t bestBits = fast, bits;
    uint32_t bestErr = 0;
    for (int t = 0; t < 16; ++t) {  // ordinal 0's error as the decoder reads the block
        const int d = ch(px, t, c) - bc4_texel((uint32_t)fast, (uint32_t)(fast >> 32), t);
        bestErr += (uint32_t)(d * d);
    }
    int mx = 0, mn = 255, lo = 255, hi = 0;  // lo / hi: over the values other than 0 and 255
    bool ends = false;
    for (int t = 0; t < 16; ++t) {
        const int v = ch(px, t, c);
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
        if (v == 0 || v == 255) {
            ends = true;
        } else {
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    for (int a = 0; a <= kBc4Inset; ++a)
        for (int b = 0; b <= kBc4Inset; ++b) {
            const int e0 = mx - a, e1 = mn + b;
            if (e0 <= e1) continue;
            const uint32_t err = bc4_assign(px, c, e0, e1, bits);
            if (err < bestErr) {  // ordinals ascend: a strict improvement only
                bestErr = err;
                bestBits = bits;
            }
        }
    if (ends && lo <= hi) {
        if (hi == lo) hi = lo + 1;  // lo <= 254
        for (int a = 0; a <= kBc4Inset; ++a)
            for (int b = 0; b <= kBc4Inset; ++b) {
                const int e0 = lo + a, e1 = hi - b;
                if (e0 >= e1) continue;
                const uint32_t err = bc4_assign(px, c, e0, e1, bits);
                if (err < bestErr) {
                    bestErr = err;
                    bestBits = bits;
                }
            }
    }
    return bestBits;
}

// one BC7 block at the quality, every candidate in ordinal order (the host's form of the wave-wide minimum)
inline void encode_bc7_host(const uint32_t *px, int quality, uint32_t out[4]) {
    if (quality == 0) {
        encode_bc7_fast(px, out);
        return;
    }
    Best best;
    const bool opaque = block_opaque(px);
    bc7_shared_candidates(px, opaque, best);
    for (int part = 0; part < 64; ++part) bc7_partition_candidates(px, part, opaque, best);
    for (int i = 0; i < 4; ++i) out[i] = best.w[i];
}

}  // namespace enc
}  // namespace bcn
}  // namespace vx
