// vxpt -- host runtime behind the C ABI (include/vxpt.h): the context's life cycle.
//
// Owns the device memory of one GPU (the reference's BufferManager /
// SkyModel / MaterialManager singletons), sets up the camera the way the
// reference does on its host (mainOffline.cpp:201-251), moves the logical
// buffers to and from the host, and holds the timing read-out and the debug
// probes.  The subsystems are in host_*.cpp, all over host_ctx.hpp.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "host_ctx.hpp"

namespace {

bool read_file(const std::string &p, std::vector<uint8_t> &out) {
    std::ifstream f(p, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

// Camera set-up exactly as mainOffline.cpp:227-246 + Camera::update (Camera.h:44-100)
V3 yaw_pitch_to_dir(float yaw, float pitch) {
    if (std::isnan(yaw) || std::isnan(pitch)) return {0, 0, 1};
    pitch = clampf(pitch, -kPiOver2 + 0.01f, kPiOver2 - 0.01f);
    const float sy = std::sin(yaw), cyw = std::cos(yaw), sp = std::sin(pitch), cp = std::cos(pitch);
    return normalize(V3(sy * cp, sp, cyw * cp));
}
CamDev make_camera_angles(int W, int H, const float pos[3], float yaw, float pitch, float fovDeg) {
    CamDev c{};
    c.res = V2((float)W, (float)H);
    c.invRes = V2(1.0f / c.res.x, 1.0f / c.res.y);
    c.pos = V3(pos[0], pos[1], pos[2]);
    const float fovX = fovDeg * kPiOver180;
    const float fovY = fovX * (c.res.y / c.res.x);
    c.tanHalfFov = V2(std::tan(fovX * 0.5f), std::tan(fovY * 0.5f));
    c.dir = yaw_pitch_to_dir(yaw, pitch);
    const V3 worldUp(0.0f, 1.0f, 0.0f);
    const V3 left = normalize(cross(worldUp, c.dir));
    const V3 up = normalize(cross(c.dir, left));
    const M3 uvToNdc = m3_cols(V3(2.0f, 0.0f, 0.0f), V3(0.0f, 2.0f, 0.0f), V3(-1.0f, -1.0f, 1.0f));
    M3 ndcToView = m3_zero();
    ndcToView.m00 = c.tanHalfFov.x;
    ndcToView.m11 = c.tanHalfFov.y;
    ndcToView.m22 = 1.0f;
    const M3 viewToWorld = m3_cols(-left, up, c.dir);
    c.uvToWorld = m3_mul(m3_mul(viewToWorld, ndcToView), uvToNdc);
    const M3 ndcToUv = m3_cols(V3(0.5f, 0.0f, 0.0f), V3(0.0f, 0.5f, 0.0f), V3(0.5f, 0.5f, 1.0f));
    const M3 worldToView = m3_transpose(viewToWorld);
    M3 viewToNdc = m3_zero();
    viewToNdc.m00 = 1.0f / c.tanHalfFov.x;
    viewToNdc.m11 = 1.0f / c.tanHalfFov.y;
    viewToNdc.m22 = 1.0f;
    c.worldToUv = m3_mul(m3_mul(ndcToUv, viewToNdc), worldToView);
    return c;
}

}  // namespace

namespace vx::host {

// the scene's direction -> yaw/pitch (DirToYawPitch) -> Camera::update
CamDev make_camera(int W, int H, const vxpt_camera &in, float *yawOut, float *pitchOut) {
    const V3 d = normalized_c(normalize(V3(in.dir[0], in.dir[1], in.dir[2])));
    const float yaw = std::atan2(d.x, d.z), pitch = std::asin(d.y);
    if (yawOut) *yawOut = yaw;
    if (pitchOut) *pitchOut = pitch;
    return make_camera_angles(W, H, in.pos, yaw, pitch, in.fov_deg);
}

CamDev make_camera_src(int W, int H, const vxpt_ctx::CamSrc &s) {
    return make_camera_angles(W, H, s.pos, s.yaw, s.pitch, s.fov);
}

// The previous camera of pose s.  After a resize that changed the aspect ratio (heldW x heldH: the size the
// history was rendered at) it keeps that size's view and takes the render size's resolution: the
// reprojection then lands on the pixel of the resampled history that holds the reprojected point.
CamDev history_camera(const vxpt_ctx *c, const vxpt_ctx::CamSrc &s) {
    if (!c->heldW) return make_camera_src(c->W, c->H, s);
    CamDev k = make_camera_src(c->heldW, c->heldH, s);
    k.res = V2((float)c->W, (float)c->H);
    k.invRes = V2(1.0f / k.res.x, 1.0f / k.res.y);
    return k;
}

// behind the frame that reprojected into the resampled history: the previous camera at the render size
void release_held_camera(vxpt_ctx *c) {
    if (!c->heldW) return;
    c->heldW = c->heldH = 0;
    if (c->prevCamSrc.set) c->prevCam = make_camera_src(c->W, c->H, c->prevCamSrc);
}

// pointer + byte size of a logical buffer
bool buffer_ptr(vxpt_ctx *c, int which, void *&p, size_t &bytes, bool forWrite, void **mirror) {
    const size_t n = (size_t)c->W * c->H;
    // current = the slot the last trace wrote; PREV_GEO_NORMAL_THIN / ALBEDO /
    // MAT_PARAM = the slot it read as the previous pass (ReSTIR history);
    // PREV_NORMAL_ROUGH / DEPTH / MATERIAL = the denoiser's history slot
    const GSlot &g = c->gb[c->last];
    const GSlot &gp = c->gb[c->tracePrev];
    const GSlot &gh = c->gb[c->hist];
    *mirror = nullptr;
    switch (which) {
        case VXPT_BUF_ILLUM: p = c->denoiseInputIsAccum ? c->accum : c->illum; bytes = n * 16; return true;
        case VXPT_BUF_DEPTH: p = g.depth; bytes = n * 4; return true;
        case VXPT_BUF_NORMAL_ROUGH: p = g.normalRough; bytes = n * 16; return true;
        case VXPT_BUF_GEO_NORMAL_THIN: p = g.geoNormalThin; bytes = n * 16; return true;
        case VXPT_BUF_PREV_GEO_NORMAL_THIN: p = gp.geoNormalThin; bytes = n * 16; return true;
        case VXPT_BUF_ALBEDO: p = g.albedo; bytes = n * 16; return true;
        case VXPT_BUF_PREV_ALBEDO: p = gp.albedo; bytes = n * 16; return true;
        case VXPT_BUF_MATERIAL: p = g.material; bytes = n * 4; return true;
        case VXPT_BUF_MAT_PARAM: p = g.matParam; bytes = n * 16; return true;
        case VXPT_BUF_PREV_MAT_PARAM: p = gp.matParam; bytes = n * 16; return true;
        case VXPT_BUF_MOTION: p = c->motion; bytes = n * 16; return true;
        case VXPT_BUF_PREV_NORMAL_ROUGH: p = gh.normalRough; bytes = n * 16; return true;
        case VXPT_BUF_PREV_DEPTH: p = gh.depth; bytes = n * 4; return true;
        case VXPT_BUF_PREV_MATERIAL: p = gh.material; bytes = n * 4; return true;
        case VXPT_BUF_RESERVOIRS: p = c->res; bytes = 2 * n * sizeof(Reservoir); return true;
        case VXPT_BUF_RES_EVEN: p = c->res; bytes = n * sizeof(Reservoir); return true;
        case VXPT_BUF_RES_ODD: p = c->res + n; bytes = n * sizeof(Reservoir); return true;
        case VXPT_BUF_WPOS: p = c->wpos; bytes = n * 16; return true;
        case VXPT_BUF_FRAME: p = c->frame; bytes = n * 16; return c->frame != nullptr;
        case VXPT_BUF_FRAME_UPSCALED:
            p = c->upscaled; bytes = (size_t)c->upW * c->upH * 16; return !forWrite && c->upW > 0;
        case VXPT_BUF_PING: p = c->ping; bytes = n * 16; return true;
        case VXPT_BUF_PONG: p = c->pong; bytes = n * 16; return true;
        case VXPT_BUF_PREV_ILLUM: p = c->prevIllum; bytes = n * 16; return true;
        case VXPT_BUF_PREV_FAST: p = c->prevFast; bytes = n * 16; return true;
        case VXPT_BUF_HIST_LEN: p = c->histLen; bytes = n * 4; return true;
        case VXPT_BUF_PREV_HIST_LEN: p = c->prevHistLen; bytes = n * 4; return true;
        case VXPT_BUF_OUTPUT: p = c->output; bytes = n * 16; return true;
        case VXPT_BUF_SKY: p = c->sky.p; bytes = 1024 * 512 * 16; return c->sky.p != nullptr;
        case VXPT_BUF_SUN: p = c->sun.p; bytes = 32 * 32 * 16; return c->sun.p != nullptr;
        case VXPT_BUF_SKY_PDF: p = c->skyPdf.p; bytes = 1024 * 512 * 4; return !forWrite && c->skyPdf.p;
        case VXPT_BUF_SUN_PDF: p = c->sunPdf.p; bytes = 32 * 32 * 4; return !forWrite && c->sunPdf.p;
        case VXPT_BUF_SUN_ALIAS: p = c->sunAlias.p; bytes = 32 * 32 * sizeof(AliasBin); return !forWrite && c->sunAlias.p;
        case VXPT_BUF_VOXELS: p = c->voxels.p; bytes = (size_t)c->cx * c->cy * c->cz * 32768; return c->voxels.p != nullptr;
        case VXPT_BUF_OCTANT_TABLES: p = c->bdist.p; bytes = (size_t)8 * c->nBricks; return !forWrite && c->bdist.p;
        case VXPT_BUF_CELL_MASKS: p = c->cellMask.p; bytes = (size_t)c->nBricks * 8; return !forWrite && c->cellMask.p;
        case VXPT_BUF_BRICK_IDS: p = c->bricks.p; bytes = (size_t)c->nBricks * 64; return !forWrite && c->bricks.p;
        case VXPT_BUF_MACRO_MASKS: p = c->macro.p; bytes = (size_t)c->nBricks / 64 * 8; return !forWrite && c->macro.p;
        case VXPT_BUF_TEXELS: p = c->texels.p; bytes = c->nTexels * 4; return !forWrite && c->texels.p && !c->texBcOn;
        case VXPT_BUF_TEX_BLOCKS:
            p = c->texBlocks.p; bytes = c->nTexBlockBytes; return !forWrite && c->texBcOn && c->texBlocks.p;
        case VXPT_BUF_BLOOM: p = c->bloomB; bytes = n * 16; return c->bloomB != nullptr;
        case VXPT_BUF_LIGHTS: p = c->lights.p; bytes = (size_t)c->nLights * sizeof(LightInfo); return !forWrite && c->nLights;
        case VXPT_BUF_TAP_RECORD: p = g.rec; bytes = n * 32; return !forWrite;
        case VXPT_BUF_CLAMP_DECISION: p = c->clampDbg; bytes = n * 4; return !forWrite && p;
        case VXPT_BUF_BOX_TABLES: p = c->bbox.p; bytes = (size_t)8 * c->nBricks * 4; return !forWrite && c->bbox.p;
        case VXPT_BUF_SKY_TOP:
            p = c->skyTop.p; bytes = (size_t)4 * (c->cx * 8) * (c->cz * 8) * 2; return !forWrite && c->skyTop.p && c->nBricks;
        case VXPT_BUF_LIGHT_ALIAS:
            p = c->lightAlias.p; bytes = (size_t)c->nLights * sizeof(AliasBin); return !forWrite && c->nLights;
        case VXPT_BUF_TLAS:
            p = c->tlas.p; bytes = (size_t)c->nTlasNodes * sizeof(BvhNode); return !forWrite && c->nMeshInst > 0;
        case VXPT_BUF_MESH_INST:
            p = c->meshInst.p; bytes = (size_t)c->nMeshInst * sizeof(MeshInst); return !forWrite && c->nMeshInst > 0;
        case VXPT_BUF_MESH_ROW_LIGHT:
            p = c->meshRowLight.p; bytes = c->instances.size() / 5 * 4; return !forWrite && !c->instances.empty() && c->meshRowLight.p;
        case VXPT_BUF_LIGHT_WEIGHT:
            p = c->lightWeight.p; bytes = (size_t)c->nLights * 4; return !forWrite && c->nLights;
        default: return false;
    }
}

}  // namespace vx::host

// =====================================================================  C ABI
extern "C" {

const char *vxpt_last_error(const vxpt_ctx *c) { return c ? c->err.c_str() : "null context"; }

int vxpt_create(const vxpt_config *cfg, vxpt_ctx **out) {
    if (!cfg || !out) return VXPT_ERR_ARG;
    *out = nullptr;
    if (cfg->width <= 0 || cfg->height <= 0) return VXPT_ERR_ARG;  // any size: partial 8x8 trace tiles and 16x16 denoise tiles are masked
    // the trace pass keeps 4 ray queues per path segment, kQueues in all (vx_internal.hpp)
    if (cfg->total_bounce_limit > kQueues / 4 || cfg->diffuse_bounce_limit > 16) return VXPT_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device) return VXPT_ERR_NODEV;
    auto *c = new vxpt_ctx();
    c->W = c->maxW = cfg->width; c->H = c->maxH = cfg->height; c->dev = cfg->device;
    c->rowBegin = cfg->row_begin; c->rowEnd = cfg->row_end;
    if (c->rowEnd <= c->rowBegin) { c->rowBegin = 0; c->rowEnd = c->H; }
    if (cfg->total_bounce_limit > 0) c->totalBounce = cfg->total_bounce_limit;
    if (cfg->diffuse_bounce_limit > 0) c->diffuseBounce = cfg->diffuse_bounce_limit;
    c->dataDir = cfg->data_dir ? cfg->data_dir : "data";
    c->yamlPost = default_post();
    c->yamlDenoise = default_denoise();
    *out = c;
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (hipStream_t &fs : c->frontStreams) HIPCHK(c, hipStreamCreateWithFlags(&fs, hipStreamNonBlocking));
    // tuning state_sets = 3: a third wavefront state set, so a first half may run beside the two
    // previous second halves (C3: 6.40 -> 6.39 ms per frame, within noise: the overlapped halves
    // already fill the chip; two sets are the default)
    for (int k = 0; k < kMaxSets; ++k)
        for (hipEvent_t *e : {&c->frontDone[k], &c->backDone[k]})
            HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(c, hipEventCreateWithFlags(&c->frontGate, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(c, hipDeviceGetAttribute(&c->numCU, hipDeviceAttributeMultiprocessorCount, c->dev));
    // timing markers only (every read of them follows a stream synchronisation): no system-scope
    // fence, so a marker neither writes back / invalidates the L2 nor delays the next kernel
    for (auto &e : c->ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    const size_t n = (size_t)c->W * c->H;
    const size_t tiles16 = (size_t)((c->W + 15) / 16) * ((c->H + 15) / 16);  // denoiser tiles
    for (auto &g : c->gb) {
        if (dalloc(c, g.normalRough, n) || dalloc(c, g.geoNormalThin, n) || dalloc(c, g.albedo, n) ||
            dalloc(c, g.matParam, n) || dalloc(c, g.depth, n) || dalloc(c, g.material, n) || dalloc(c, g.rec, 2 * n))
            return VXPT_ERR_HIP;
    }
    if (dalloc(c, c->illum, n) || dalloc(c, c->accum, n) || dalloc(c, c->motion, n) || dalloc(c, c->res, 2 * n) ||
        dalloc(c, c->ping, n) || dalloc(c, c->pong, n) || dalloc(c, c->prevIllum, n) || dalloc(c, c->prevFast, n) ||
        dalloc(c, c->output, n) || dalloc(c, c->histLen, n) || dalloc(c, c->prevHistLen, n) ||
        dalloc(c, c->wpos, n) || dalloc(c, c->ffCount, tiles16) || dalloc(c, c->ffIndex, tiles16 * 256) ||
        dalloc(c, c->ffColor, tiles16 * 256) || dalloc(c, c->ffRes, tiles16 * 256) ||
        dalloc(c, c->ffCand, tiles16 * 256) || dalloc(c, c->ffCandCount, 1) ||
        dalloc(c, c->hfList, tiles16 * 256) || dalloc(c, c->hfCount, tiles16))
        return VXPT_ERR_HIP;
    c->illumSet[0] = c->illum;
    c->accumBuf[0] = c->accum;
    if (dalloc(c, c->accumBuf[1], n)) return VXPT_ERR_HIP;
    for (int k = 1; k < kMaxSets; ++k)  // (a third set's plane too: vxpt_set_tuning may enable it)
        if (dalloc(c, c->illumSet[k], n)) return VXPT_ERR_HIP;
    // tables
    const std::string t = c->dataDir + "/tables/";
    std::vector<uint8_t> so, sc, rk, f0, f1, f2, f3;
    if (!read_file(t + "bn_sobol.u8", so) || !read_file(t + "bn_scramble.u8", sc) || !read_file(t + "bn_rank.u8", rk) ||
        !read_file(t + "sky_datasets.f32", f0) || !read_file(t + "sky_datasets_rad.f32", f1) ||
        !read_file(t + "solar_datasets.f32", f2) || !read_file(t + "limb_darkening.f32", f3) ||
        so.size() != 65536 || sc.size() != 131072 || rk.size() != 131072 || f0.size() != 2160 || f1.size() != 240 ||
        f2.size() != 7200 || f3.size() != 240)
        return fail(c, VXPT_ERR_IO, "cannot read tables from " + t);
    if (upload_vec(c, c->bnSobol, so.data(), so.size()) || upload_vec(c, c->bnScramble, sc.data(), sc.size()) ||
        upload_vec(c, c->bnRank, rk.data(), rk.size()) ||
        upload_vec(c, c->solar, (const float *)f2.data(), 1800) || upload_vec(c, c->limb, (const float *)f3.data(), 60))
        return VXPT_ERR_HIP;
    std::memcpy(c->tabSky, f0.data(), sizeof(c->tabSky));
    std::memcpy(c->tabSkyRad, f1.data(), sizeof(c->tabSkyRad));
    // default material table: terrain materials of data/assets/materials.yaml
    const float rough[13] = {0.5f, 0.8f, 0.9f, 0.85f, 0.9f, 0.8f, 0.7f, 0.85f, 0.6f, 0.7f, 0.65f, 0.75f, 0.75f};
    for (int b = 1; b <= 12; ++b) c->mats[b] = MatDev{{1.f, 1.f, 1.f}, rough[b], 0.0f, 0, b - 1, 0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

void vxpt_destroy(vxpt_ctx *c) {
    if (!c) return;
    hipSetDevice(c->dev);
    for (hipStream_t fs : c->frontStreams)
        if (fs) hipStreamSynchronize(fs);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (void *p : c->allocs) hipFree(p);
    for (int k = 0; k < kMaxSets; ++k)
        for (hipEvent_t e : {c->frontDone[k], c->backDone[k]})
            if (e) hipEventDestroy(e);
    if (c->frontGate) hipEventDestroy(c->frontGate);
    for (hipStream_t fs : c->frontStreams)
        if (fs) hipStreamDestroy(fs);
    for (hipEvent_t e : c->chainEv) hipEventDestroy(e);
    for (hipEvent_t e : c->bst.pool) hipEventDestroy(e);
    for (auto &e : c->ev)
        if (e) hipEventDestroy(e);
    for (auto &e : c->runEv)
        if (e) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->commStream) hipStreamDestroy(c->commStream);
    if (c->haloReady) hipEventDestroy(c->haloReady);
    if (c->haloDone) hipEventDestroy(c->haloDone);
    if (c->exDone) hipEventDestroy(c->exDone);
    for (hipEvent_t e : c->upEv)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->rzEv)
        if (e) hipEventDestroy(e);
    if (c->skyWritten) hipEventDestroy(c->skyWritten);
    if (c->hSkyHeads) hipHostFree(c->hSkyHeads);
    for (hipEvent_t e : {c->worldWritten, c->editDone[0], c->editDone[1], c->wbEv[0], c->wbEv[1]})
        if (e) hipEventDestroy(e);
    for (WbRec *p : c->editStage)
        if (p) hipHostFree(p);
    for (hipEvent_t e : c->terEv)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : {c->instWritten, c->ibEv[0], c->ibEv[1], c->bcEv[0], c->bcEv[1]})
        if (e) hipEventDestroy(e);
    for (auto &s : c->instStage) {
        if (s.done) hipEventDestroy(s.done);
        if (s.p) hipHostFree(s.p);
    }
    delete c;
}

int vxpt_set_camera(vxpt_ctx *c, const vxpt_camera *cur, const vxpt_camera *prev) {
    if (!c || !cur) return VXPT_ERR_ARG;
    c->cam = make_camera(c->W, c->H, *cur, &c->camYaw, &c->camPitch);
    const vxpt_camera &pv = prev ? *prev : *cur;
    float pyaw, ppitch;
    c->prevCam = make_camera(c->W, c->H, pv, &pyaw, &ppitch);
    c->camSrc = {{cur->pos[0], cur->pos[1], cur->pos[2]}, c->camYaw, c->camPitch, cur->fov_deg, true};
    c->prevCamSrc = {{pv.pos[0], pv.pos[1], pv.pos[2]}, pyaw, ppitch, pv.fov_deg, true};
    if (c->heldW) c->prevCam = history_camera(c, c->prevCamSrc);
    return VXPT_OK;
}

int vxpt_set_camera_angles(vxpt_ctx *c, const float pos[3], float yaw, float pitch, float fovDeg) {
    if (!c || !pos) return VXPT_ERR_ARG;
    c->prevCam = c->cam;  // historyCamera = camera (mainOffline.cpp:278-279)
    c->prevCamSrc = c->camSrc;
    if (c->heldW && c->prevCamSrc.set) c->prevCam = history_camera(c, c->prevCamSrc);
    c->cam = make_camera_angles(c->W, c->H, pos, yaw, pitch, fovDeg);
    c->camSrc = {{pos[0], pos[1], pos[2]}, yaw, pitch, fovDeg, true};
    c->camYaw = yaw;
    c->camPitch = pitch;
    return VXPT_OK;
}

int vxpt_get_camera(vxpt_ctx *c, int which, float *o) {
    if (!c || !o) return VXPT_ERR_ARG;
    const CamDev &k = which ? c->prevCam : c->cam;
    const float v[32] = {k.pos.x, k.pos.y, k.pos.z, k.dir.x, k.dir.y, k.dir.z,
                         k.uvToWorld.m00, k.uvToWorld.m10, k.uvToWorld.m20, k.uvToWorld.m01, k.uvToWorld.m11,
                         k.uvToWorld.m21, k.uvToWorld.m02, k.uvToWorld.m12, k.uvToWorld.m22,
                         k.worldToUv.m00, k.worldToUv.m10, k.worldToUv.m20, k.worldToUv.m01, k.worldToUv.m11,
                         k.worldToUv.m21, k.worldToUv.m02, k.worldToUv.m12, k.worldToUv.m22,
                         k.res.x, k.res.y, k.invRes.x, k.invRes.y, k.tanHalfFov.x, k.tanHalfFov.y, c->camYaw, c->camPitch};
    std::memcpy(o, v, sizeof(v));
    return VXPT_OK;
}

int vxpt_readback(vxpt_ctx *c, int which, void *host, size_t bytes) {
    if (!c || !host) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    void *p, *mirror;
    size_t n;
    if (!buffer_ptr(c, which, p, n, false, &mirror)) return fail(c, VXPT_ERR_ARG, "unknown buffer");
    if (bytes < n) return fail(c, VXPT_ERR_ARG, "host buffer too small");
    HIPCHK(c, hipMemcpyAsync(host, p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

int vxpt_upload(vxpt_ctx *c, int which, const void *host, size_t bytes) {
    if (!c || !host) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    void *p, *mirror;
    size_t n;
    if (which == VXPT_BUF_FRAME)  // an image to upscale need not come from vxpt_postprocess
        if (int r = post_alloc(c)) return r;
    // sky, sun and voxels are derived state: set them through their own entry points
    if (!buffer_ptr(c, which, p, n, true, &mirror) || (which >= 32 && which <= 34))
        return fail(c, VXPT_ERR_ARG, "unknown or read-only buffer");
    if (bytes < n) return fail(c, VXPT_ERR_ARG, "host buffer too small");
    gbuf_written(c, which);
    HIPCHK(c, hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, c->stream));
    if (mirror) HIPCHK(c, hipMemcpyAsync(mirror, host, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

int vxpt_timings(vxpt_ctx *c, vxpt_timing *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    if (int r = sky_resolve(c)) return r;
    *out = c->timing;
    return VXPT_OK;
}

int vxpt_device_memory(vxpt_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    size_t f = 0, t = 0;
    HIPCHK(c, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return VXPT_OK;
}

int vxpt_sync(vxpt_ctx *c) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

void *vxpt_stream(vxpt_ctx *c) { return c ? (void *)c->stream : nullptr; }

}  // extern "C"

// probe kernel lives in trace.hip
namespace vx {
hipError_t launch_probe(const WorldDev &w, int n, const float *rays, int *out, float *t, int mode, hipStream_t st);
}

extern "C" int vxpt_probe_rays(vxpt_ctx *c, int n, const float *rays, int32_t *out6, float *t, int mode) {
    if (!c || n <= 0 || !rays || !out6 || !t) return VXPT_ERR_ARG;
    if (!c->voxels.p) return fail(c, VXPT_ERR_STATE, "no voxels");
    HIPCHK(c, hipSetDevice(c->dev));
    float *dr;
    int *dout;
    float *dt;
    HIPCHK(c, hipMalloc(&dr, (size_t)n * 8 * 4));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 6 * 4));
    HIPCHK(c, hipMalloc(&dt, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(dr, rays, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    WorldDev w;
    fill_world(c, w);
    HIPCHK(c, launch_probe(w, n, dr, dout, dt, mode, c->stream));
    HIPCHK(c, hipMemcpyAsync(out6, dout, (size_t)n * 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(t, dt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dr);
    hipFree(dout);
    hipFree(dt);
    return VXPT_OK;
}

extern "C" int vxpt_trace_counters(vxpt_ctx *c, uint32_t *out, int cap) {
    if (!c || !out || cap < 48) return VXPT_ERR_ARG;
    if (!c->wb[c->lastSet].qCount) return fail(c, VXPT_ERR_STATE, "no trace buffers");
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<uint32_t> q(kQueueWords);
    HIPCHK(c, hipMemcpyAsync(q.data(), c->wb[c->lastSet].qCount, q.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 16; ++k) {
        out[3 * k] = q[k];
        for (int level = 1; level <= 2; ++level) {
            uint32_t n = 0;
            for (int sh = 0; sh < kShards; ++sh) n += q[2 * kQueues + (((level - 1) * kQueues + k) * kShards + sh) * 16];
            out[3 * k + level] = n;
        }
    }
    return VXPT_OK;
}

extern "C" int vxpt_probe_rng(vxpt_ctx *c, int n, const int32_t *q4, float *out) {
    if (!c || n <= 0 || !q4 || !out) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    int *dq;
    float *dout;
    HIPCHK(c, hipMalloc(&dq, (size_t)n * 16));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 4));
    HIPCHK(c, hipMemcpyAsync(dq, q4, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    const BlueNoiseDev bn{c->bnSobol.p, c->bnScramble.p, c->bnRank.p};
    HIPCHK(c, launch_probe_rng(bn, n, dq, dout, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(dq);
    hipFree(dout);
    return VXPT_OK;
}
