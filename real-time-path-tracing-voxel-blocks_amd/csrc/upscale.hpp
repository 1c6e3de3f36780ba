// Render-scale filters, one body for the host (vxpt_upscale_host) and the device (upscale.hip):
// the edge-adaptive spatial upsampler (ScalingFilter.h:124-342), the contrast-adaptive sharpener
// (SharpeningFilter.h:33-63) and the Catmull-Rom resampler (BicubicFilter.h:5-27 over
// Sampler.h:500-574).  Everything is fp32 on the RGB of a float4 image; the library is built with
// -ffp-contract=off and IEEE division and square root, and minima / maxima are spelled as
// compares, so both sides produce the same bits.
//
// A body reads its texels through a fetch object `t`: t.rgb(dx, dy) and t.lum(dx, dy) are the
// colour and the luminance of the texel (dx, dy) away from the body's anchor texel, edge-clamped by
// whoever built the object (the host clamps indices, the kernel clamps while it stages LDS).
//
// Deviations from the reference kernels: fp32 instead of packed half; exact 1/x and
// 1/sqrt(x); the luminance of texel X feeds slot X; true bilinear weights of the four direction
// estimates; a flat difference pair contributes no length; a weight sum of 0 yields texel f; the
// sharpener takes its strength as a parameter, writes out of place and passes a flat 3x3
// neighbourhood through; the Catmull-Rom sum is taken over differences from tap (1, 1).
#pragma once
#include "vx_math.hpp"

namespace vx {
namespace upscale {

// vxpt_upscale_mode (include/vxpt.h)
constexpr int kBicubic = 0, kEasu = 1, kEasuSharpen = 2;

VX_HD float mn(float a, float b) { return b < a ? b : a; }
VX_HD float mx(float a, float b) { return b > a ? b : a; }
VX_HD V3 mn3(V3 a, V3 b) { return V3(mn(a.x, b.x), mn(a.y, b.y), mn(a.z, b.z)); }
VX_HD V3 mx3(V3 a, V3 b) { return V3(mx(a.x, b.x), mx(a.y, b.y), mx(a.z, b.z)); }
VX_HD float easu_lum(V3 c) { return c.x * 0.5f + (c.y + c.z * 0.5f); }

// output pixel -> input position: p = i * scale + bias per axis (con0 of the reference)
struct Map {
    float sx, sy, bx, by;
};
VX_HD Map make_map(int w, int h, int ow, int oh) {
    Map m;
    m.sx = (float)w / (float)ow;
    m.sy = (float)h / (float)oh;
    m.bx = 0.5f * m.sx - 0.5f;
    m.by = 0.5f * m.sy - 0.5f;
    return m;
}
// texel f of an output column / row and the position's fraction inside it
VX_HD int easu_anchor(int i, float scale, float bias, float &frac) {
    const float p = (float)i * scale + bias;
    const float f = floorf(p);
    frac = p - f;
    return (int)f;
}

// FsrEasuSetH for one of the texels f, g, j, k: the + pattern (a above, b left, c centre, d right,
// e below) in luminance, bilinear weight w
VX_HD void easu_set(float &dirX, float &dirY, float &len, float w, float lA, float lB, float lC, float lD, float lE) {
    const float dc = lD - lC, cb = lC - lB;
    const float mX = mx(fabsf(dc), fabsf(cb));
    const float dX = lD - lB;
    dirX += dX * w;
    float lenX = mX > 0.0f ? clampf(fabsf(dX) * (1.0f / mX), 0.0f, 1.0f) : 0.0f;
    lenX *= lenX;
    len += lenX * w;
    const float ec = lE - lC, ca = lC - lA;
    const float mY = mx(fabsf(ec), fabsf(ca));
    const float dY = lE - lA;
    dirY += dY * w;
    float lenY = mY > 0.0f ? clampf(fabsf(dY) * (1.0f / mY), 0.0f, 1.0f) : 0.0f;
    lenY *= lenY;
    len += lenY * w;
}

struct EasuKernel {
    float dirX, dirY, len2X, len2Y, lob, clp;
};
// FsrEasuTapH: one tap at offset (ox, oy) from the sample position
VX_HD void easu_tap(V3 &aC, float &aW, float ox, float oy, const EasuKernel &k, V3 c) {
    float vX = ox * k.dirX + oy * k.dirY;
    float vY = ox * (-k.dirY) + oy * k.dirX;
    vX *= k.len2X;
    vY *= k.len2Y;
    const float d2 = mn(vX * vX + vY * vY, k.clp);
    float wB = (2.0f / 5.0f) * d2 + -1.0f;
    float wA = k.lob * d2 + -1.0f;
    wB *= wB;
    wA *= wA;
    wB = (25.0f / 16.0f) * wB + -(25.0f / 16.0f - 1.0f);
    const float w = wB * wA;
    aC += c * w;
    aW += w;
}

// The upsampler for one output pixel; t is anchored at texel f, (px, py) the position's fraction
//      b c
//    e f g h
//    i j k l
//      n o
template <class T>
VX_HD V3 easu(const T &t, float px, float py) {
    const float bL = t.lum(0, -1), cL = t.lum(1, -1);
    const float eL = t.lum(-1, 0), fL = t.lum(0, 0), gL = t.lum(1, 0), hL = t.lum(2, 0);
    const float iL = t.lum(-1, 1), jL = t.lum(0, 1), kL = t.lum(1, 1), lL = t.lum(2, 1);
    const float nL = t.lum(0, 2), oL = t.lum(1, 2);
    // the reference's two packed lanes: (f then j) and (g then k), summed at the end
    float dx0 = 0.0f, dy0 = 0.0f, ln0 = 0.0f, dx1 = 0.0f, dy1 = 0.0f, ln1 = 0.0f;
    easu_set(dx0, dy0, ln0, (1.0f - px) * (1.0f - py), bL, eL, fL, gL, jL);
    easu_set(dx1, dy1, ln1, px * (1.0f - py), cL, fL, gL, hL, kL);
    easu_set(dx0, dy0, ln0, (1.0f - px) * py, fL, iL, jL, kL, nL);
    easu_set(dx1, dy1, ln1, px * py, gL, jL, kL, lL, oL);
    float dirX = dx0 + dx1, dirY = dy0 + dy1, len = ln0 + ln1;

    float dirR = dirX * dirX + dirY * dirY;
    const bool zro = dirR < (1.0f / 32768.0f);
    dirR = zro ? 1.0f : 1.0f / sqrtf(dirR);
    dirX = zro ? 1.0f : dirX;
    dirX *= dirR;
    dirY *= dirR;
    len = len * 0.5f;
    len = len * len;
    const float stretch = (dirX * dirX + dirY * dirY) * (1.0f / mx(fabsf(dirX), fabsf(dirY)));
    EasuKernel k;
    k.dirX = dirX;
    k.dirY = dirY;
    k.len2X = 1.0f + (stretch - 1.0f) * len;
    k.len2Y = 1.0f + -0.5f * len;
    k.lob = 0.5f + ((1.0f / 4.0f - 0.04f) - 0.5f) * len;
    k.clp = 1.0f / k.lob;

    const V3 cF = t.rgb(0, 0), cG = t.rgb(1, 0), cJ = t.rgb(0, 1), cK = t.rgb(1, 1);
    const V3 lo = mn3(mn3(cF, cG), mn3(cJ, cK)), hi = mx3(mx3(cF, cG), mx3(cJ, cK));
    V3 a0(0.0f), a1(0.0f);
    float w0 = 0.0f, w1 = 0.0f;
    easu_tap(a0, w0, 0.0f - px, -1.0f - py, k, t.rgb(0, -1));  // b
    easu_tap(a1, w1, 1.0f - px, -1.0f - py, k, t.rgb(1, -1));  // c
    easu_tap(a0, w0, -1.0f - px, 1.0f - py, k, t.rgb(-1, 1));  // i
    easu_tap(a1, w1, 0.0f - px, 1.0f - py, k, cJ);             // j
    easu_tap(a0, w0, 0.0f - px, 0.0f - py, k, cF);             // f
    easu_tap(a1, w1, -1.0f - px, 0.0f - py, k, t.rgb(-1, 0));  // e
    easu_tap(a0, w0, 1.0f - px, 1.0f - py, k, cK);             // k
    easu_tap(a1, w1, 2.0f - px, 1.0f - py, k, t.rgb(2, 1));    // l
    easu_tap(a0, w0, 2.0f - px, 0.0f - py, k, t.rgb(2, 0));    // h
    easu_tap(a1, w1, 1.0f - px, 0.0f - py, k, cG);             // g
    easu_tap(a0, w0, 1.0f - px, 2.0f - py, k, t.rgb(1, 2));    // o
    easu_tap(a1, w1, 0.0f - px, 2.0f - py, k, t.rgb(0, 2));    // n
    const V3 aC = a0 + a1;
    const float aW = w0 + w1;
    if (aW == 0.0f) return cF;
    return mn3(hi, mx3(lo, aC * (1.0f / aW)));
}

// The sharpener for one pixel; t is anchored at the pixel (only rgb is read)
template <class T>
VX_HD V3 sharpen(const T &t, float sharpness) {
    const V3 c = t.rgb(0, 0), w = t.rgb(-1, 0), e = t.rgb(1, 0), n = t.rgb(0, -1), s = t.rgb(0, 1);
    const V3 nw = t.rgb(-1, -1), ne = t.rgb(1, -1), sw = t.rgb(-1, 1), se = t.rgb(1, 1);
    const V3 hiP = mx3(mx3(mx3(c, w), mx3(e, n)), s), hiA = mx3(mx3(hiP, mx3(nw, ne)), mx3(sw, se));
    const V3 loP = mn3(mn3(mn3(c, w), mn3(e, n)), s), loA = mn3(mn3(loP, mn3(nw, ne)), mn3(sw, se));
    const V3 sum = ((w + e) + n) + s;
    const float peak = 8.0f - 3.0f * sharpness;
    V3 out;
    for (int i = 0; i < 3; ++i) {
        const float softmax = hiP.get(i) + hiA.get(i), softmin = loP.get(i) + loA.get(i);
        float r = c.get(i);
        if (softmax > 0.0f && loA.get(i) != hiA.get(i)) {
            const float amp = clampf(mn(softmin, 2.0f - softmax) / softmax, 0.0f, 1.0f);
            const float wt = -sqrtf(amp) / peak;
            r = (sum.get(i) * wt + r) / (1.0f + 4.0f * wt);
        }
        out.set(i, r);
    }
    return out;
}

// Catmull-Rom weights of the four taps around a fraction f (Sampler.h:513-516)
VX_HD void catmull_rom(float f, float w[4]) {
    const float f2 = f * f, f3 = f2 * f;
    w[0] = f2 - 0.5f * (f3 + f);
    w[1] = 1.5f * f3 - 2.5f * f2 + 1.0f;
    w[3] = 0.5f * (f3 - f2);
    w[2] = 1.0f - w[0] - w[1] - w[3];
}
// tap (1, 1) of an output column / row (tc1 of the reference) and the fraction past it
VX_HD int bicubic_anchor(int i, int outSize, int texSize, float &frac) {
    const float uv = ((float)i + 0.5f) / (float)outSize;
    const float UV = uv * (float)texSize;
    const float fl = floorf(UV - 0.5f);
    frac = UV - (fl + 0.5f);
    return (int)fl;
}
// SampleBicubicCatmullRom for one output pixel; t is anchored at tap (1, 1).  The weighted sum runs
// over the taps' differences from that tap, so a constant image is reproduced exactly.
template <class T>
VX_HD V3 bicubic(const T &t, float fx, float fy) {
    float wx[4], wy[4];
    catmull_rom(fx, wx);
    catmull_rom(fy, wy);
    const V3 c = t.rgb(0, 0);
    V3 acc(0.0f);
    float sum = 0.0f;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            const float w = wx[i] * wy[j];
            sum += w;
            acc += (t.rgb(i - 1, j - 1) - c) * w;
        }
    return c + acc / sum;
}

// ---- the host's fetch objects: edge-clamped reads of a float4 image
struct HostTex {
    const float *img;
    int w, h, x, y;
    VX_HD V3 rgb(int dx, int dy) const {
        const float *p = img + 4 * ((size_t)clampi(y + dy, 0, h - 1) * w + clampi(x + dx, 0, w - 1));
        return V3(p[0], p[1], p[2]);
    }
    VX_HD float lum(int dx, int dy) const { return easu_lum(rgb(dx, dy)); }
};

}  // namespace upscale

// launcher (upscale.hip): in = W x H float4, out = outW x outH float4, Float4(rgb, 0); tmp = as out, the
// upsampled image the sharpener reads (mode 2 only)
hipError_t launch_upscale(const float4 *in, int W, int H, float4 *out, float4 *tmp, int outW, int outH, int mode,
                          float sharpness, hipStream_t st);
// the same bodies on the host
void upscale_host(const float *in, int w, int h, float *out, int ow, int oh, int mode, float sharpness);

}  // namespace vx
