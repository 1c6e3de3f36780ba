// vxpt -- host runtime, the sky: Vose's alias tables on the host, the sky model's fitted state, the sky and sun
// maps with their tables built on the host or on the device (sky.hip), the alias probe.
#include <algorithm>
#include <cmath>
#include <queue>
#include <vector>

#include "host_ctx.hpp"

namespace vx::host {

std::vector<AliasBin> build_alias(const std::vector<float> &w, float &sumOut) {
    const unsigned n = (unsigned)w.size();
    double acc = 0.0;
    for (unsigned i = 0; i < n; ++i) acc += (double)w[i];
    const float sum = (float)acc;
    sumOut = sum;
    std::vector<float> prob(n), scaled(n);
    std::vector<int> alias(n, -1);
    for (unsigned i = 0; i < n; ++i) {
        prob[i] = w[i] / sum;
        scaled[i] = prob[i] * n;
    }
    std::queue<int> small, large;
    for (unsigned i = 0; i < n; ++i) (scaled[i] < 1.0f ? small : large).push((int)i);
    while (!small.empty() && !large.empty()) {
        const int s = small.front(); small.pop();
        const int l = large.front(); large.pop();
        alias[s] = l;
        scaled[l] -= (1.0f - scaled[s]);
        (scaled[l] < 1.0f ? small : large).push(l);
    }
    while (!small.empty()) { scaled[small.front()] = 1.0f; small.pop(); }
    while (!large.empty()) { scaled[large.front()] = 1.0f; large.pop(); }
    std::vector<AliasBin> b(n);
    for (unsigned i = 0; i < n; ++i) b[i] = {scaled[i], prob[i], alias[i]};
    return b;
}

}  // namespace vx::host

namespace {

float fit6(const float *M, float t, int i, int stride) {  // Sky.cu:19-47
    return (std::pow(1.0f - t, 5.0f) * M[i] + 5.0f * std::pow(1.0f - t, 4.0f) * t * M[i + stride] +
            10.0f * std::pow(1.0f - t, 3.0f) * std::pow(t, 2.0f) * M[i + 2 * stride] +
            10.0f * std::pow(1.0f - t, 2.0f) * std::pow(t, 3.0f) * M[i + 3 * stride] +
            5.0f * (1.0f - t) * std::pow(t, 4.0f) * M[i + 4 * stride] + std::pow(t, 5.0f) * M[i + 5 * stride]);
}

V3 q_rotate3(V3 axis, float angle, V3 v) {  // rotate3f (LinearMath.h:1368)
    const Qt q{normalized_c(axis) * std::sin(angle / 2), std::cos(angle / 2)};
    return q_mul(q_mul(q, {v, 0.f}), q_conj(q)).v;
}

}  // namespace

extern "C" {

namespace {

constexpr int kSkyW = 1024, kSkyH = 512, kSunW = 32, kSunH = 32;

// the sun direction (Sky.cu:363-368) into the context and the sky model's fitted state
// (updateSkyState, Sky.cu:57-83, CPU fit); the maps and pdf planes on the first call
int sky_state(vxpt_ctx *c, float tod, float axisAngle, float axisRotate, float cfg[90], float rad[10]) {
    V3 axis(1.0f, std::cos(axisAngle * kPiOver180), std::sin(axisAngle * kPiOver180));
    axis *= V3(std::sin(axisRotate * kPiOver180), 1.0f, std::cos(axisRotate * kPiOver180));
    axis = normalize(axis);
    const float angle = std::fmod(tod * kPi, kTwoPi);
    c->sunDir = normalized_c(q_rotate3(axis, angle, cross(V3(0, 1, 0), axis)));
    const float elevation = (kPi / 2.0f) - std::acos(c->sunDir.y);
    const float se = std::pow(elevation / (kPi / 2.0f), (1.0f / 3.0f));
    for (int ch = 0; ch < 10; ++ch) {
        for (int i = 0; i < 9; ++i) cfg[ch * 9 + i] = fit6(c->tabSky + ch * 54, se, i, 9);
        rad[ch] = fit6(c->tabSkyRad + ch * 6, se, 0, 1);
    }
    const int sw = kSkyW, sh = kSkyH, uw = kSunW, uh = kSunH;
    if (!c->sky.p) {
        if (dalloc(c, c->sky.p, (size_t)sw * sh) || dalloc(c, c->sun.p, (size_t)uw * uh) ||
            dalloc(c, c->skyPdf.p, (size_t)sw * sh) || dalloc(c, c->sunPdf.p, (size_t)uw * uh))
            return VXPT_ERR_HIP;
        c->sky.n = (size_t)sw * sh; c->sun.n = (size_t)uw * uh;
    }
    return 0;
}

}  // namespace

// the alias kernels' scratch for n bins (at least the sky table's, so that the sky builds and the
// probes up to that size share one allocation), the heads, and the build event: once per context
int alias_scratch(vxpt_ctx *c, int n) {
    if (!c->skyHeads) {
        if (dalloc(c, c->skyHeads, 4)) return VXPT_ERR_HIP;
        HIPCHK(c, hipHostMalloc((void **)&c->hSkyHeads, 3 * sizeof(AliasHead), hipHostMallocDefault));
        HIPCHK(c, hipEventCreate(&c->skyWritten));
    }
    AliasScratch &s = c->aliasScratch;
    if (s.cap >= n) return 0;
    const size_t cap = (size_t)std::max(n, kSkyW * kSkyH);
    if (dalloc(c, s.part, cap / ab::kChunk + 1) || dalloc(c, s.blk, cap / ab::kChunk + 1) || dalloc(c, s.D, cap + 1) ||
        dalloc(c, s.E, cap) || dalloc(c, s.light, cap) || dalloc(c, s.heavy, cap))
        return VXPT_ERR_HIP;
    s.cap = (int)cap;
    return 0;
}

// what a device sky build left for the host: the sun table's sum and the build's time (one wait for
// the build's event; nothing to do after a host build)
int sky_resolve(vxpt_ctx *c) {
    if (!c->skyPending) return 0;
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipEventSynchronize(c->skyWritten));
    c->sunLuminance = c->hSkyHeads[2].fsum;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[4], c->ev[5]);
    c->timing.sky_ms = ms;
    c->skyPending = false;
    return 0;
}

int vxpt_set_sky(vxpt_ctx *c, float tod, float axisAngle, float axisRotate, float brightness) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    float cfg[90], rad[10];
    if (int r = sky_state(c, tod, axisAngle, axisRotate, cfg, rad)) return r;
    const int sw = kSkyW, sh = kSkyH, uw = kSunW, uh = kSunH;
    c->skyPending = false;
    c->skyDevice = false;
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    HIPCHK(c, launch_sky(cfg, rad, c->solar.p, c->limb.p, c->sunDir, brightness, c->sky.p, c->sun.p, c->skyPdf.p,
                         c->sunPdf.p, sw, sh, uw, uh, c->stream));
    std::vector<float> pdf((size_t)sw * sh), spdf((size_t)uw * uh);
    HIPCHK(c, hipMemcpyAsync(pdf.data() + (size_t)sw * (sh / 2), c->skyPdf.p + (size_t)sw * (sh / 2),
                             (size_t)sw * (sh / 2) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double upper = 0.0;
    for (size_t i = (size_t)sw * (sh / 2); i < (size_t)sw * sh; ++i) upper += (double)pdf[i];
    HIPCHK(c, launch_sky_lower(c->sky.p, c->skyPdf.p, sw, sh, (float)upper, c->stream));
    HIPCHK(c, hipMemcpyAsync(pdf.data(), c->skyPdf.p, pdf.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(spdf.data(), c->sunPdf.p, spdf.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float s1, s2;
    c->hSkyAlias = build_alias(pdf, s1);
    const std::vector<AliasBin> sunA = build_alias(spdf, s2);
    c->sunLuminance = s2;
    if (upload_vec(c, c->skyAlias, c->hSkyAlias.data(), c->hSkyAlias.size()) ||
        upload_vec(c, c->sunAlias, sunA.data(), sunA.size()))
        return VXPT_ERR_HIP;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[4], c->ev[5]);
    c->timing.sky_ms = ms;
    c->skyReady = true;
    return VXPT_OK;
}

int vxpt_set_sky_device(vxpt_ctx *c, float tod, float axisAngle, float axisRotate, float brightness) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    float cfg[90], rad[10];
    if (int r = sky_state(c, tod, axisAngle, axisRotate, cfg, rad)) return r;
    const int sw = kSkyW, sh = kSkyH, uw = kSunW, uh = kSunH;
    if (int r = alias_scratch(c, sw * sh)) return r;
    if (grow(c, c->skyAlias, (size_t)sw * sh) || grow(c, c->sunAlias, (size_t)uw * uh)) return VXPT_ERR_HIP;
    // every earlier first half has finished before the context stream gets here: its second half, which
    // waited for it, was enqueued on this stream
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    HIPCHK(c, launch_sky(cfg, rad, c->solar.p, c->limb.p, c->sunDir, brightness, c->sky.p, c->sun.p, c->skyPdf.p,
                         c->sunPdf.p, sw, sh, uw, uh, c->stream));
    const size_t half = (size_t)sw * (sh / 2);
    HIPCHK(c, launch_tree_sum(c->skyPdf.p + half, (int)half, c->aliasScratch, c->skyHeads + 0, c->stream));
    HIPCHK(c, launch_sky_lower_dev(c->sky.p, c->skyPdf.p, sw, sh, c->skyHeads + 0, c->stream));
    HIPCHK(c, launch_alias_build(c->skyPdf.p, sw * sh, c->aliasScratch, c->skyHeads + 1, c->skyAlias.p, c->stream));
    HIPCHK(c, launch_alias_build(c->sunPdf.p, uw * uh, c->aliasScratch, c->skyHeads + 2, c->sunAlias.p, c->stream));
    // the one readback: the sun table's sum is a kernel argument of the post-process (sun_projection)
    HIPCHK(c, hipMemcpyAsync(c->hSkyHeads, c->skyHeads, 3 * sizeof(AliasHead), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    // written: the passes' first halves read the maps and tables on the front streams
    HIPCHK(c, hipEventRecord(c->skyWritten, c->stream));
    for (hipStream_t fs : c->frontStreams)
        if (fs) HIPCHK(c, hipStreamWaitEvent(fs, c->skyWritten, 0));
    c->hSkyAlias.clear();
    c->skyDevice = true;
    c->skyPending = true;
    c->skyReady = true;
    return VXPT_OK;
}

int vxpt_alias_build_host(const float *w, int n, float *q, float *p, int32_t *alias, float *sum) {
    return ab::build_host(w, n, q, p, alias, sum) ? VXPT_OK : VXPT_ERR_ARG;
}

int vxpt_alias_build(vxpt_ctx *c, const float *w, int n, float *q, float *p, int32_t *alias, float *sum) {
    if (!c || !w || n < 1 || n > ab::kMaxN) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    if (int r = alias_scratch(c, n)) return r;
    float *dw;
    AliasBin *dout;
    HIPCHK(c, hipMalloc(&dw, (size_t)n * 4));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * sizeof(AliasBin)));
    std::vector<AliasBin> bins(n);
    AliasHead head{};
    HIPCHK(c, hipMemcpyAsync(dw, w, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_alias_build(dw, n, c->aliasScratch, c->skyHeads + 3, dout, c->stream));
    HIPCHK(c, hipMemcpyAsync(bins.data(), dout, (size_t)n * sizeof(AliasBin), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&head, c->skyHeads + 3, sizeof(head), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dw);
    hipFree(dout);
    for (int i = 0; i < n; ++i) {
        if (q) q[i] = bins[i].q;
        if (p) p[i] = bins[i].p;
        if (alias) alias[i] = bins[i].alias;
    }
    if (sum) *sum = head.fsum;
    return VXPT_OK;
}

int vxpt_get_sky_alias(vxpt_ctx *c, float *q, float *p, int32_t *alias, float *sunDir) {
    if (!c || !c->skyReady) return VXPT_ERR_STATE;
    if (c->skyDevice && c->hSkyAlias.empty()) {  // a device-built table: read back on demand
        HIPCHK(c, hipSetDevice(c->dev));
        c->hSkyAlias.resize((size_t)kSkyW * kSkyH);
        HIPCHK(c, hipMemcpyAsync(c->hSkyAlias.data(), c->skyAlias.p, c->hSkyAlias.size() * sizeof(AliasBin),
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (size_t i = 0; i < c->hSkyAlias.size(); ++i) {
        if (q) q[i] = c->hSkyAlias[i].q;
        if (p) p[i] = c->hSkyAlias[i].p;
        if (alias) alias[i] = c->hSkyAlias[i].alias;
    }
    if (sunDir) { sunDir[0] = c->sunDir.x; sunDir[1] = c->sunDir.y; sunDir[2] = c->sunDir.z; }
    return VXPT_OK;
}

}  // extern "C"
