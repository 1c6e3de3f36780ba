// The denoiser's two stages in front of temporal accumulation, one body for the host
// (vxpt_prefilter_host) and the device (denoise.hip):
//   hit-distance reconstruction  HitDistReconstruction<8,2> (HitDistReconstruction.h:51-162)
//   pre-pass blur                PrePass (PrePass.h:6-150)
// Everything is fp32; the library is built with -ffp-contract=off and IEEE division and square root,
// and neither body calls a transcendental function: the reference's ExpApprox is rational
// (DenoiserCommon.h:62-70), and every term that needs exp / atan / sin / cos is launch-uniform and
// computed once on the host (Consts, make_consts).  So both sides produce the same bits, and a tap
// coordinate -- an integer decision -- is the same on both.
//
// A body reads its inputs through a fetch object.  The reconstruction's `t` is anchored at the pixel:
// t.nrm(dx, dy), t.hd(dx, dy), t.vz(dx, dy) are the normal, the hit distance (radiance w) and |depth| of
// the edge-clamped texel (dx, dy) away (the host clamps indices, the kernel clamps while it stages
// LDS: HitDistReconstruction.h:30).  The pre-pass's `p` is indexed by plane index, -1 for a tap outside
// the screen, which reads zeros and fetches nothing: p.z(i), p.mat(i), p.nrm(i), p.rad(i).
//
// Both stages hard-code the reference's constants (denoisingRange 500000, depthThreshold 0.003,
// lobeAngleFraction 0.5: HitDistReconstruction.h:41,99, PrePass.h:39,86,120); they do not read
// vxpt_denoise_params.  Deviations from the reference kernels: DESIGN.md §9.2.
#pragma once
#include <algorithm>
#include <cmath>

#include "vx_internal.hpp"

namespace vx {
namespace prefilter {

constexpr float kRange = 500000.0f;
constexpr int kStageHitDist = 0, kStagePrePass = 1;  // vxpt_prefilter_host's stage

// launch-uniform terms
struct Consts {
    float gauss5[9];     // reconstruction: GetGaussianWeight(length(o) * 0.5) by |o|^2 (DenoiserCommon.h:48-51)
    float nwpRecon;      // GetNormalWeightParams(1, 1, 1) (HitDistReconstruction.h:11-17,111)
    float rotCa, rotSa;  // GetRotator(Weyl1D(0.5, iterationIndex) * radians(90)) (PrePass.h:49-50)
    float gauss8[8];     // pre-pass: GetGaussianWeight(g_Poisson8[i].z) (PrePass.h:139)
    float nwpPre;        // GetNormalWeightParam2(1, 0.25 * lobeAngleFraction) (PrePass.h:89)
    float hdA;           // GetHitDistanceWeightParams(., 1 / 9).x (PrePass.h:90, DenoiserCommon.h:397-405)
    float frustumK;      // camera.getPixelWorldSizeScaleToDepth() (Camera.h:128-131)
    float invW, invH;    // invScreenResolution (Denoiser.cu:28)
    float minWH;         // min(screenResolution.x, screenResolution.y) (PrePass.h:78)
};

VX_HD V3 poisson8(int i) {  // g_Poisson8 (PrePass.h:63-72)
    const float p[8][3] = {{-0.4706069f, -0.4427112f, +0.6461146f}, {-0.9057375f, +0.3003471f, +0.9542373f},
                           {-0.3487388f, +0.4037880f, +0.5335386f}, {+0.1023042f, +0.6439373f, +0.6520134f},
                           {+0.5699277f, +0.3513750f, +0.6695386f}, {+0.2939128f, -0.1131226f, +0.3149309f},
                           {+0.7836658f, -0.4208784f, +0.8895339f}, {+0.1564120f, -0.8198990f, +0.8346850f}};
    return V3(p[i][0], p[i][1], p[i][2]);
}

// host only: the transcendental terms (the same libm call feeds the kernel's arguments and the host body)
inline Consts make_consts(const CamDev &cam, int W, int H, int iterationIndex) {
    Consts k;
    for (int d2 = 0; d2 <= 8; ++d2) {
        const float r = std::sqrt((float)d2) * 0.5f;
        k.gauss5[d2] = std::exp(-0.66f * r * r);
    }
    // GetSpecularLobeHalfAngle(1): atan(m * 0.75f / (1.0 - 0.75f)) in double, the angle a float
    // (DenoiserCommon.h:27-31); scaled by lerp(1, 1, 1) = 1; 1.0 / max(angle, 0.5 deg) in double
    const float angle = (float)std::atan((double)(1.0f * 0.75f) / (1.0 - (double)0.75f));
    k.nwpRecon = (float)(1.0 / (double)angle);
    // Weyl1D(0.5, n) = fract(0.5 + float(n * 10368889) / 2^24) (DenoiserCommon.h:336-339; the int
    // product wraps), radians(90) = 90 * (M_PI / 180.0f) in double (LinearMath.h:2012-2015)
    const int32_t prod = (int32_t)((uint32_t)iterationIndex * 10368889u);
    float ip;
    const float weyl = std::modf(0.5f + (float)prod / 16777216.0f, &ip);
    const float a1 = weyl * (float)(90.0 * (3.14159265358979323846 / (double)180.0f));
    k.rotCa = std::cos(a1);
    k.rotSa = std::sin(a1);
    for (int i = 0; i < 8; ++i) {
        const float z = poisson8(i).z;
        k.gauss8[i] = std::exp(-0.66f * z * z);
    }
    // GetSpecLobeTanHalfAngle(1, 0.125), GetNormalWeightParam2 (DenoiserCommon.h:366-382)
    const float pv = 0.25f * 0.5f;
    const float tanHalf = 1.0f * 1.0f * pv / (1.0f - pv + 1e-6f);
    k.nwpPre = 1.0f / std::max(std::atan(tanHalf), 1e-6f);
    // GetSpecMagicCurve(1) = (1 - 2^-200) * 1^0.25 = 1, so norm = lerp(0.0005, 1, min(1 / 9, 1))
    const float norm = 0.0005f + (1.0f / 9.0f) * (1.0f - 0.0005f);
    k.hdA = 1.0f / norm;
    k.frustumK = cam.tanHalfFov.x / (cam.res.x / 2);
    k.invW = 1.0f / (float)W;
    k.invH = 1.0f / (float)H;
    k.minWH = (float)(W < H ? W : H);
    return k;
}

VX_HD float acos_approx(float x) { return 1.41421356f * sqrtf(saturate(1.0f - x)); }  // DenoiserCommon.h:33-36
// ComputeExponentialWeight over ExpApprox(x) = rcp(x * x - x + 1) (DenoiserCommon.h:62-70)
VX_HD float exp_weight(float x, float px, float py, float scale) {
    const float v = -scale * fabsf(x * px + py);
    return 1.0f / ((v * v - v) + 1.0f);
}
// GetBilateralWeight: LinearStep(0.03, 0, |z - zc| / (max(|z|, |zc|) + 1e-6)) (DenoiserCommon.h:53-60)
VX_HD float bilateral_weight(float z, float zc) {
    const float t = fabsf(z - zc) * (1.0f / (fmaxf(fabsf(z), fabsf(zc)) + 1e-6f));
    return saturate((t - 0.03f) / (0.0f - 0.03f));
}
// ComputeNonExponentialWeight = SmoothStep(1, 0, |x * px + py|) (DenoiserCommon.h:11-15,351-354)
VX_HD float nonexp_weight(float x, float px, float py) {
    const float t = saturate((fabsf(x * px + py) - 1.0f) / (0.0f - 1.0f));
    return t * t * (3.0f - 2.0f * t);
}
VX_HD V3 pixel_world_pos(const CamDev &c, int x, int y, float depth) {  // DenoiserCommon.h:272-279
    const V2 uv = (V2((float)x, (float)y) + 0.5f) * c.invRes;
    return c.pos + c.uv_to_dir(uv) * depth;
}

// The reconstructed hit distance of one pixel inside the denoising range
// (HitDistReconstruction.h:103-156).  IsInScreen(pixelUv + o / res) (:134) is the integer test: the
// uv of an in-screen texel centre lies 0.5 / res inside [0, 1], far more than its rounding.
template <class T>
VX_HD float hitdist_px(const T &t, const Consts &k, int W, int H, int x, int y) {
    const V3 cN = t.nrm(0, 0);
    const float cHd = t.hd(0, 0), cVz = t.vz(0, 0);
    float sumW = 1000.0f * (cHd != 0.0f ? 1.0f : 0.0f);
    float sum = cHd * sumW;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float angle = acos_approx(saturate(dot(cN, t.nrm(dx, dy))));
            const int sx = x + dx, sy = y + dy;
            float w = (sx >= 0 && sy >= 0 && sx < W && sy < H) ? 1.0f : 0.0f;
            w *= k.gauss5[dx * dx + dy * dy];
            w *= bilateral_weight(t.vz(dx, dy), cVz);
            float dw = w;
            dw *= exp_weight(angle, k.nwpRecon, 0.0f, 3.0f);
            const float sHd = dw == 0.0f ? 0.0f : t.hd(dx, dy);  // Denanify
            dw *= sHd != 0.0f ? 1.0f : 0.0f;
            sum += sHd * dw;
            sumW += dw;
        }
    return sum / fmaxf(sumW, 1e-6f);
}

// The pre-pass's blur radius in pixels (PrePass.h:77-84): 30 * saturate(hitDist / frustumSize), at
// least 1 where the centre's hit distance is 0
VX_HD float blur_radius(const Consts &k, float viewZ, float hitDist) {
    const float frustum = k.minWH * k.frustumK * viewZ;
    const float hd = hitDist == 0.0f ? 1.0f : hitDist;
    float r = 30.0f * saturate(hd / frustum);
    if (hitDist == 0.0f) r = fmaxf(r, 1.0f);
    return r;
}
// Texel of tap i (PrePass.h:98-105): floor(pixelUv * res + RotateVector(rotator, offset.xy) * radius),
// in the reference's operation order.  Geometry and radiance are both read there.
VX_HD void tap_texel(const Consts &k, int W, int H, int x, int y, float radius, int i, int &ix, int &iy) {
    const V3 o = poisson8(i);
    const float ux = ((float)x + 0.5f) * k.invW * (float)W, uy = ((float)y + 0.5f) * k.invH * (float)H;
    const float rx = o.x * k.rotCa + o.y * k.rotSa, ry = o.x * (-k.rotSa) + o.y * k.rotCa;
    ix = (int)floorf(ux + rx * radius);
    iy = (int)floorf(uy + ry * radius);
}
VX_HD int tap_index(int W, int H, int ix, int iy) {  // -1: outside the screen (IsInScreenNearest, PrePass.h:116)
    return (ix >= 0 && iy >= 0 && ix < W && iy < H) ? iy * W + ix : -1;
}

// The blurred radiance of one pixel inside the denoising range (PrePass.h:43-147).  c: its radiance
// and hit distance, cz / cMat / cN: its depth, material and normal.  Every tap's four values are
// fetched before the first weight.  The accumulation keeps the reference's Float4 operators
// (vx_math.hpp V4): `sample * weight` puts z * weight into w, and `/= weightSum` adds weightSum to w.
template <class P>
VX_HD V4 prepass_px(const P &p, const CamDev &cam, const Consts &k, int W, int H, int x, int y, V4 c, float cz,
                    float cMat, V3 cN) {
    const V3 cWP = pixel_world_pos(cam, x, y, cz);
    const float radius = blur_radius(k, cz, c.w);
    const float hdB = c.w * k.hdA;  // GetHitDistanceWeightParams: (a, -hitDist * a)
    int tx[8], ty[8], idx[8];
    float sz[8], sm[8];
    V3 sn[8];
    V4 sv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        tap_texel(k, W, H, x, y, radius, i, tx[i], ty[i]);
        idx[i] = tap_index(W, H, tx[i], ty[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sz[i] = p.z(idx[i]);
        sm[i] = p.mat(idx[i]);
        sn[i] = p.nrm(idx[i]);
        sv[i] = p.rad(idx[i]);
    }
    float weightSum = 1.0f;
    V4 sum = c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float w = idx[i] >= 0 ? 1.0f : 0.0f;
        w *= sz[i] < kRange ? 1.0f : 0.0f;
        w *= cMat == sm[i] ? 1.0f : 0.0f;
        const V3 sWP = pixel_world_pos(cam, tx[i], ty[i], sz[i]);
        w *= fabsf(dot(sWP - cWP, cN)) / cz > 0.003f ? 0.0f : 1.0f;  // GetPlaneDistanceWeight
        w *= nonexp_weight(acos_approx(dot(cN, sn[i])), k.nwpPre, 0.0f);
        const V4 s = w == 0.0f ? V4() : sv[i];  // Denanify
        w *= lerpf(0.2f, 1.0f, exp_weight(s.w, k.hdA, -hdB, 3.0f));
        w *= k.gauss8[i];
        weightSum += w;
        sum += s * w;
    }
    sum /= weightSum;
    return sum;
}

// ---- the host's fetch objects
struct HostHit {
    const float *illum, *depth, *normalRough;
    int w, h, x, y;
    VX_HD size_t at(int dx, int dy) const { return (size_t)clampi(y + dy, 0, h - 1) * w + clampi(x + dx, 0, w - 1); }
    VX_HD V3 nrm(int dx, int dy) const {
        const float *n = normalRough + 4 * at(dx, dy);
        return V3(n[0], n[1], n[2]);
    }
    VX_HD float hd(int dx, int dy) const { return illum[4 * at(dx, dy) + 3]; }
    VX_HD float vz(int dx, int dy) const { return fabsf(depth[at(dx, dy)]); }
};
struct HostPre {
    const float *in, *depth, *normalRough, *material;
    VX_HD float z(int i) const { return i < 0 ? 0.0f : depth[i]; }
    VX_HD float mat(int i) const { return i < 0 ? 0.0f : material[i]; }
    VX_HD V3 nrm(int i) const {
        return i < 0 ? V3(0.0f) : V3(normalRough[4 * (size_t)i], normalRough[4 * (size_t)i + 1], normalRough[4 * (size_t)i + 2]);
    }
    VX_HD V4 rad(int i) const {
        return i < 0 ? V4() : V4(in[4 * (size_t)i], in[4 * (size_t)i + 1], in[4 * (size_t)i + 2], in[4 * (size_t)i + 3]);
    }
};

}  // namespace prefilter

// launchers (denoise.hip), whole frames only.  Reconstruction: a.illum -> a.ping.  Pre-pass: reads
// a.ping when fromPing, else a.illum, which is first copied to a.ping (the pass must not run in place,
// and the ping plane is scratch then); writes a.illum.
hipError_t launch_hitdist(const DenoiseArgs &a, hipStream_t st);
hipError_t launch_prepass(const DenoiseArgs &a, int iterationIndex, bool fromPing, hipStream_t st);
// the same bodies on the host: planes of w * h pixels (illum and normalRough float4, depth and material
// float), out = w * h float4; tapXY (may be null, pre-pass only) = the 8 taps' texels (x, y) per pixel
void prefilter_host(int stage, const CamDev &cam, int w, int h, int iterationIndex, const float *illum,
                    const float *depth, const float *normalRough, const float *material, float *out, int32_t *tapXY);

}  // namespace vx
