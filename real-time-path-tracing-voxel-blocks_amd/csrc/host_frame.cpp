// vxpt -- host runtime, the frame: a trace pass's two halves on their streams, the denoiser chain and its single
// passes, the frame loops (OfflineBackend.cpp:46-89), post-processing, upscaling and the pre-filter's host twin.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host_ctx.hpp"
#include "prefilter.hpp"
#include "upscale.hpp"

namespace vx::host {

void fill_world(vxpt_ctx *c, WorldDev &w) {
    w.ids = c->voxels.p;
    w.bricks = c->bricks.p;
    w.macro = c->macro.p;
    w.cellMask = c->cellMask.p;
    w.bdist = c->bdist.p;
    w.bbox = c->useBoxes ? c->bbox.p : nullptr;
    w.nBricks = c->nBricks;
    // a brick walk yields its lanes back to the outer loop after brick_steps (3) crossings (fewer lanes
    // idle behind long in-brick walks; C3 trace 6.44 -> 6.26 ms per frame)
    w.brickSteps = c->tune.brick_steps;
    w.brickStepsCam = c->tune.cam_steps;
    w.top = c->top;
    w.topValid = c->topValid;
    w.skyTop = c->tune.sky_exit ? c->skyTop.p : nullptr;
    w.brickPass = c->tune.brick_pass;
    w.cx = c->cx; w.cy = c->cy; w.cz = c->cz;
    w.wx = c->cx * 32; w.wy = c->cy * 32; w.wz = c->cz * 32;
    w.mx = w.wx / 16; w.my = w.wy / 16; w.mz = w.wz / 16;
    w.tx = (w.wx + 63) / 64; w.ty = (w.wy + 63) / 64; w.tz = (w.wz + 63) / 64;
}

}  // namespace vx::host

namespace {

void fill_sky(vxpt_ctx *c, SkyDev &s) {
    s.sky = c->sky.p;
    s.sun = c->sun.p;
    s.skyAlias = c->skyAlias.p;
    s.sunAlias = c->sunAlias.p;
    s.sunDir = c->sunDir;
    s.skyW = 1024; s.skyH = 512; s.sunW = 32; s.sunH = 32;
    s.sunCosMax = std::cos(0.51f * kPi / 180.0f / 2.0f);
}

void fill_denoise(vxpt_ctx *c, const vxpt_denoise_params *p, DenoiseArgs &a, int parity) {
    a.W = c->W; a.H = c->H;
    a.y0 = c->rowBegin; a.y1 = c->rowEnd;
    a.cam = c->cam; a.prevCam = c->prevCam;
    a.p = {p->max_accumulated_frame_num, p->max_fast_accumulated_frame_num, p->phi_luminance,
           p->lobe_angle_fraction, p->roughness_fraction, p->depth_threshold, p->disocclusion_threshold,
           p->disocclusion_threshold_alternate, p->denoising_range, p->enable_temporal_accumulation,
           p->enable_history_fix, p->enable_history_clamping, p->enable_spatial_filtering,
           p->enable_firefly_filter, p->atrous_iteration_num, p->enable_hit_distance_reconstruction,
           p->enable_pre_pass};
    const GSlot &g = c->gb[c->last];
    a.illum = c->denoiseInputIsAccum ? c->accum : c->illum;
    a.normalRough = g.normalRough;
    a.albedo = g.albedo;
    a.motion = c->motion;
    a.depth = g.depth;
    a.material = g.material;
    a.prevNormalRough = c->gb[c->hist].normalRough;
    a.prevDepth = c->gb[c->hist].depth;
    a.reservoir = c->res + (size_t)parity * c->W * c->H;
    a.ping = c->ping; a.pong = c->pong; a.prevIllum = c->prevIllum; a.prevFast = c->prevFast;
    a.output = c->output;
    a.histLen = c->histLen; a.prevHistLen = c->prevHistLen;
    a.ffCount = c->ffCount; a.ffIndex = c->ffIndex; a.ffColor = c->ffColor; a.ffRes = c->ffRes;
    a.ffCand = c->ffCand; a.ffCandCount = c->ffCandCount;
    a.hfList = c->hfList; a.hfCount = c->hfCount;
    a.wpos = c->wpos;
    a.clampDbg = c->clampDbgOn ? c->clampDbg : nullptr;
    a.invW = 1.0f / (float)c->W; a.invH = 1.0f / (float)c->H;
    a.thrB = a.p.disocclusionThreshold + (1.5f / (float)c->H);
    a.thrA = a.p.disocclusionThresholdAlternate + (1.5f / (float)c->H);
    a.frustumK = c->cam.tanHalfFov.x / (c->cam.res.x / 2);
    a.invAcc1 = 1.0f / (a.p.maxAcc + 1.0f);
    a.invFast1 = 1.0f / (a.p.maxFast + 1.0f);
    a.tune.ffFused = c->tune.firefly_fused;
    a.tune.taSupertiles = c->tune.ta_supertiles;
    a.tune.hfSplit = c->tune.hf_split;
    a.tune.stencilTile = c->tune.stencil_tile;
}

// wavefront trace state of one set for ns slots (8x8 tiles of the band), 4 visibility rays per slot;
// allocated at the first pass that needs it (a band context holds its band's slots only).  The
// allocation's zero fill is enqueued on the context stream: `fresh` tells the caller
int ensure_wave(vxpt_ctx *c, int set, size_t ns, bool &fresh) {
    fresh = false;
    if (c->wbSlots[set] >= ns) return 0;
    fresh = true;
    // a whole-frame context allocates for the created size, so that a render size that grows back finds room
    if (!is_banded(c)) ns = std::max(ns, (size_t)((c->maxW + 7) / 8) * ((c->maxH + 7) / 8) * 64);
    WaveBufs &w = c->wb[set];
    w = WaveBufs{};  // a smaller earlier set stays allocated (freed with the context)
    if (dalloc(c, w.pPos, ns) || dalloc(c, w.pDir, ns) || dalloc(c, w.pThr, ns) || dalloc(c, w.pRad, ns) ||
        dalloc(c, w.pMeta, ns) || dalloc(c, w.pBop, ns) || dalloc(c, w.cRayO, ns) || dalloc(c, w.cRayD, ns) ||
        dalloc(c, w.cHit, ns) || dalloc(c, w.cT, ns) || dalloc(c, w.sPos, ns) || dalloc(c, w.sNrm, ns) ||
        dalloc(c, w.sGeo, ns) || dalloc(c, w.sAlb, ns) || dalloc(c, w.sWo, ns) || dalloc(c, w.cSunSky, ns) ||
        dalloc(c, w.rRis, ns) || dalloc(c, w.rRR, ns) || dalloc(c, w.nIdx, ns) ||
        dalloc(c, w.ls0, ns) || dalloc(c, w.ls1, ns) || dalloc(c, w.tapPsv, ns) || dalloc(c, w.tapM, ns) ||
        dalloc(c, w.oHit, 4 * ns) ||
        dalloc(c, w.qO, 4 * ns) || dalloc(c, w.qD, 4 * ns) ||
        dalloc(c, w.qId, 4 * ns) || dalloc(c, w.qCount, kQueueWords) ||
        dalloc(c, w.sCell[0], 4 * ns + 2048) || dalloc(c, w.sT[0], 4 * ns + 2048) ||
        dalloc(c, w.sFace[0], 4 * ns + 2048) || dalloc(c, w.sCell[1], 4 * ns + 2048) ||
        dalloc(c, w.sT[1], 4 * ns + 2048) || dalloc(c, w.sFace[1], 4 * ns + 2048) ||
        dalloc(c, w.sBack, ns) || dalloc(c, w.rLoc, ns) || dalloc(c, w.lLoc0, ns) || dalloc(c, w.lLoc1, ns))
        return VXPT_ERR_HIP;
    c->wbSlots[set] = ns;
    return 0;
}

// history hand-over NormalRough/Depth/Material -> Prev (Denoiser.cu:394-407):
// the slot the frame's last trace wrote becomes the denoiser's history slot
// (whole planes, so the rows a band received from its neighbours come along)
hipError_t history_copies(vxpt_ctx *c) {
    c->histOld = c->hist;
    c->hist = c->last;
    return hipSuccess;
}

// world positions for the band and kWposHalo rows either side (the widest
// stencil, HistoryFix at 2 x 17 rows, reads them there), in the firefly pass's
// launch (`detect`: the filter over the band; `apply`: write the filtered pixels
// back in this launch rather than in the next k_temporal)
hipError_t firefly_band(const DenoiseArgs &a, bool detect, bool apply, hipStream_t st) {
    return launch_firefly(a, std::max(0, a.y0 - kWposHalo), std::min(a.H, a.y1 + kWposHalo), detect, apply, st);
}

}  // namespace

namespace vx::host {

// One 1-spp pass, first half.  overlap: the first half may run beside the previous pass's second
// half (it then waits only for the pass before that to release its state set).  Otherwise it starts
// after everything enqueued on the context stream.  A primary-only pass runs whole on the context
// stream here.
hipStream_t front_stream(const vxpt_ctx *c, int set) { return c->frontStreams[set % c->tune.front_streams]; }

// planes = false: a frame's pass before its last, which writes its tap records but not the G-buffer
// planes (the frame's planes are its last pass's; nothing reads an earlier pass's)
int trace_front(vxpt_ctx *c, int32_t it, uint32_t flags, bool accumulate, bool accumFirst, float accumScale,
                bool overlap, PassPlan &pl, bool planes) {
    if (!c->voxels.p) return fail(c, VXPT_ERR_STATE, "no voxels uploaded");
    if (!c->skyReady) return fail(c, VXPT_ERR_STATE, "sky not set");
    TraceArgs a{};
    fill_world(c, a.world);
    fill_sky(c, a.sky);
    a.bn = {c->bnSobol.p, c->bnScramble.p, c->bnRank.p};
    for (int i = 0; i < 13; ++i) a.mats[i] = c->mats[i];
    if (c->nMeshInst > 0) {
        if (!c->meshMats.p || std::memcmp(c->meshMatsUp, c->mats, sizeof(c->mats)) != 0) {
            if (int r = upload_vec(c, c->meshMats, c->mats, 32)) return r;
            std::memcpy(c->meshMatsUp, c->mats, sizeof(c->mats));
            overlap = false;  // the first half reads them: after the upload
        }
        a.mesh = mesh_dev(c);
        a.meshUV = c->blasUV.p;
        a.meshRow = c->meshRow.p;
        a.meshRowLight = c->meshRowLight.p;
        a.meshMats = c->meshMats.p;
        a.lights = c->lights.p;
        a.lightAlias = c->lightAlias.p;
        a.numLights = (int)c->nLights;
    }
    a.cam = c->cam;
    // the temporal taps reproject into the previous pass's view: the frame's history camera for its
    // first pass, the frame's own camera for the later passes of an accumulation
    a.prevCam = (accumulate && !accumFirst) ? c->cam : c->prevCam;
    // the slot this pass writes: not the previous pass's (its temporal taps), not the denoiser's
    // history, and not the one the previous pass's second half may still be reading
    int next = 0;
    while (next == c->last || next == c->hist || next == c->histOld || next == c->tracePrev || next == c->tracePrev2)
        ++next;
    const GSlot &cur = c->gb[next], &prev = c->gb[c->last];
    a.cur = {cur.normalRough, cur.geoNormalThin, cur.albedo, cur.matParam, cur.depth, cur.material, cur.rec};
    a.prev = {prev.normalRough, prev.geoNormalThin, prev.albedo, prev.matParam, prev.depth, prev.material, prev.rec};
    if (prev.recStale) {  // planes uploaded or copied in from the host: rebuild the taps' records
        HIPCHK(c, launch_pack_rec(a.prev, (size_t)c->W * c->H, c->stream));
        c->gb[c->last].recStale = false;
    }
    c->gb[next].recStale = false;  // this pass writes the records (and the planes unless !planes)
    const int set = c->passCount % c->nSets;
    a.illum = c->illumSet[set];
    a.motion = c->motion;
    a.writeMotion = c->motionZero ? 0 : 1;
    a.writePlanes = (planes || (flags & VXPT_TRACE_PRIMARY_ONLY)) ? 1 : 0;
    const size_t n = (size_t)c->W * c->H;
    a.resCur = c->res + (size_t)(((it % 2) + 2) % 2) * n;
    a.resPrev = c->res + (size_t)((((it + 1) % 2) + 2) % 2) * n;
    // the first pass of an accumulation writes the other buffer (the previous accumulation, the
    // pipelined denoiser's input, stays intact); trace_back makes it current
    a.accum = accumulate ? (accumFirst ? (c->accum == c->accumBuf[0] ? c->accumBuf[1] : c->accumBuf[0]) : c->accum)
                         : nullptr;
    a.accumScale = accumScale;
    a.accumFirst = accumFirst ? 1 : 0;
    a.W = c->W; a.H = c->H;
    a.y0 = c->rowBegin; a.y1 = c->rowEnd;
    a.iterationIndex = it;
    a.totalBounceLimit = c->totalBounce;
    a.diffuseBounceLimit = c->diffuseBounce;
    // A path outlives its first segment only through a specular hit (roughness
    // <= 1e-5, closesthit.cu:224) or a diffuse limit above 1 (RayGen.cu:146-173);
    // otherwise the later segments' kernels would find no live path.
    bool anySpecular = false;
    for (int b = 1; b <= 12; ++b) anySpecular |= !(c->mats[b].roughness > 0.00001f);
    if (c->nMeshInst > 0)  // instanced meshes in the world: their materials count too
        for (int b = 13; b < kBlockTypes; ++b)
            anySpecular |= c->blocks[b].triangles > 0 && !c->mats[b].emissive && !(c->mats[b].roughness > 0.00001f);
    a.segments = (c->diffuseBounce == 1 && !anySpecular) ? 1 : c->totalBounce;
    a.primaryOnly = (flags & VXPT_TRACE_PRIMARY_ONLY) ? 1 : 0;
    a.tilesX = (c->W + 7) / 8;
    a.nSlots = a.tilesX * ((a.y1 - a.y0 + 7) / 8) * 64;
    // tuning overlap = 0 (diagnostics): every first half after the previous pass, kernels one at a time
    if (!c->tune.overlap) overlap = false;
    bool fresh;
    if (int r = ensure_wave(c, set, (size_t)a.nSlots, fresh)) return r;
    if (fresh) overlap = false;  // the first half must follow the new buffers' zero fill
    a.wb = c->wb[set];
    a.numCU = c->numCU;
    a.iterCap = c->tune.iter_cap;
    a.iterCap2 = c->tune.iter_cap2;
    a.iterCap3 = c->tune.iter_cap3;
    a.iterCap4 = c->tune.iter_cap4;
    a.resumeWgPerCU = c->tune.resume_wg_per_cu;
    a.sortMode = c->tune.sort_mode;
    a.ldsBricks = c->tune.lds_bricks;
    a.resumeSplit = c->tune.resume_split;
    a.laterSplit = c->tune.later_split;
    a.restirWaves = c->tune.restir_waves;
    // whole 4-tile workgroups per tile row for the panels
    a.xcdOrder = c->tune.xcd_order & (a.tilesX % 4 == 0 ? 7 : 4);
    a.prevSceneEmpty = c->prevSceneEmpty;
    // the one pass after a light update remaps the previous pass's light indices (OptixRenderer.cpp:447-457)
    a.lightsDirty = (c->lightsDirty && c->prevNumLights > 0) ? 1 : 0;
    a.prevNumLights = (int)c->prevNumLights;
    a.lightRemap = c->lightRemap.p;
    // a primary-only pass runs no temporal reuse: the remap waits for the next full pass
    if (!(flags & VXPT_TRACE_PRIMARY_ONLY)) c->lightsDirty = 0;
    a.tex = c->texTable.p;
    a.texels = c->texels.p;
    a.texEnabled = (c->texEnabled && c->texTable.p) ? 1 : 0;
    a.texBc = c->texBcOn ? c->texBcTable.p : nullptr;
    a.texBlocks = c->texBcOn ? c->texBlocks.p : nullptr;
    c->prevSceneEmpty = 0;
    if (a.primaryOnly) {
        HIPCHK(c, launch_trace_front(a, c->stream));
    } else {
        // first half on its front stream: after the pass that last used this state set (overlap), or
        // after everything on the context stream
        hipStream_t fs = front_stream(c, set);
        if (overlap) {
            HIPCHK(c, hipStreamWaitEvent(fs, c->backDone[set], 0));
        } else {
            HIPCHK(c, hipEventRecord(c->frontGate, c->stream));
            HIPCHK(c, hipStreamWaitEvent(fs, c->frontGate, 0));
        }
        HIPCHK(c, launch_trace_front(a, fs));
        HIPCHK(c, hipEventRecord(c->frontDone[set], fs));
    }
    pl.a = a;
    pl.next = next;
    pl.set = set;
    return 0;
}

// Pipelined frames: whether a frame's later first halves wait (on the host) for the previous frame's
// denoiser chain.  Nothing requires it when spp >= 2 and the motion plane is the static world's: a
// first half writes a G-buffer slot that excludes the two the chain reads (hist, histOld), its own state
// set and radiance plane (the chain reads the spp average), and the motion plane only after an upload
// of it.  Otherwise (tuning chain_gate, the default) the gate keeps the chain alone on the GPU.
bool chain_gate(const vxpt_ctx *c, int spp) { return c->tune.chain_gate || spp < 2 || !c->motionZero; }

// The second half of the planned pass, on the context stream, and the ring bookkeeping.
// mark: record ev[1] behind the pass (vxpt_trace's timing; the frame loops keep their own events --
// every marker is one more packet between two kernels of the stream)
int trace_back(vxpt_ctx *c, const PassPlan &pl, bool mark) {
    const int set = pl.set;
    if (!pl.a.primaryOnly) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->frontDone[set], 0));
        HIPCHK(c, launch_trace_back(pl.a, c->stream, c->haloPending ? c->haloDone : nullptr));
        HIPCHK(c, hipEventRecord(c->backDone[set], c->stream));
    }
    c->haloPending = false;
    if (mark) HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    c->tracePrev2 = c->tracePrev;
    c->tracePrev = c->last;
    c->last = pl.next;
    c->illum = c->illumSet[set];
    if (pl.a.accum) c->accum = pl.a.accum;
    c->lastSet = set;
    ++c->passCount;
    return 0;
}

int do_trace(vxpt_ctx *c, int32_t it, uint32_t flags, bool accumulate, bool accumFirst, float accumScale,
             bool overlap, bool mark, bool planes) {
    if (mark) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    PassPlan pl;
    if (int r = trace_front(c, it, flags, accumulate, accumFirst, accumScale, overlap, pl, planes)) return r;
    return trace_back(c, pl, mark);
}

// Denoiser::run (Denoiser.cu:24-408) on the context stream.  (Running all of it but the firefly
// stage on a third stream beside the next frame's first pass was measured and removed)
// The two stages in front of temporal accumulation have no band schedule (the pre-pass reaches 30 rows,
// the reconstruction 2: a halo group of their own): the switch a banded call must refuse
const char *prefilter_switch(const vxpt_denoise_params *p) {
    if (p->enable_hit_distance_reconstruction) return "enable_hit_distance_reconstruction";
    if (p->enable_pre_pass) return "enable_pre_pass";
    return nullptr;
}
int refuse_prefilter(vxpt_ctx *c, const char *sw) {
    return fail(c, VXPT_ERR_STATE, (std::string(sw) + " is not supported on banded contexts (a row range, a band "
                                    "communicator or linked contexts)").c_str());
}
bool is_banded(const vxpt_ctx *c) { return c->rowBegin != 0 || c->rowEnd != c->H || c->comm || !c->linked.empty(); }

int do_denoise(vxpt_ctx *c, const vxpt_denoise_params *p, int frameNum, int it) {
    p = denoise_or_yaml(c, p);
    const bool recon = p->enable_hit_distance_reconstruction != 0, pre = p->enable_pre_pass != 0;
    if ((recon || pre) && is_banded(c)) return refuse_prefilter(c, prefilter_switch(p));
    const int used = it > 0 ? it - 1 : 0;
    DenoiseArgs a{};
    fill_denoise(c, p, a, used & 1);
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    // the temporal pass applies the firefly lists when it runs
    // (the two optional stages read the filtered radiance: the firefly pass then applies its own lists)
    const bool ffFold = p->enable_temporal_accumulation && frameNum > 0 && !recon && !pre;
    HIPCHK(c, firefly_band(a, p->enable_firefly_filter, !ffFold, c->stream));
    hipStream_t st = c->stream;
    int fin = 0;  // 0 illum, 1 ping, 2 pong, 3 prevIllum
    // Denoiser.cu:79-92: the reconstruction alone moves the result to the ping plane; :101-119: the
    // pre-pass reads this frame's radiance (the reconstruction's output if it ran) and writes illum
    if (recon) { HIPCHK(c, launch_hitdist(a, st)); fin = 1; }
    if (pre) HIPCHK(c, launch_prepass(a, it, recon, st));
    if (frameNum == 0) HIPCHK(c, launch_frame0_init(a, st));
    if (p->enable_temporal_accumulation && frameNum > 0) {
        HIPCHK(c, launch_temporal(a, st));
        fin = 1;
        if (p->enable_history_fix) { HIPCHK(c, launch_history_fix(a, st)); fin = 2; }
        if (p->enable_history_clamping) { HIPCHK(c, launch_history_clamp(a, st)); fin = 3; }
    }
    bool outputDone = false;
    if (p->enable_spatial_filtering) {
        HIPCHK(c, launch_atrous_smem(a, st));
        fin = 1;
        if (p->atrous_iteration_num > 0) {
            int idx = 1;
            unsigned step = 1u << idx;
            const int maxIt = p->atrous_iteration_num * 2;
            while (idx < maxIt) {
                HIPCHK(c, launch_atrous(a, a.ping, a.pong, step, (unsigned)it, false, st));
                ++idx; step = 1u << idx;
                HIPCHK(c, launch_atrous(a, a.pong, a.ping, step, (unsigned)it, false, st));
                ++idx; step = 1u << idx;
            }
            HIPCHK(c, launch_atrous(a, a.ping, a.pong, step, (unsigned)it, true, st));
            fin = 2;
            outputDone = true;
        }
    }
    if (!outputDone) {
        const float4 *src = fin == 1 ? a.ping : (fin == 2 ? a.pong : (fin == 3 ? a.prevIllum : a.illum));
        HIPCHK(c, launch_copy_output(a, src, st));
    }
    HIPCHK(c, history_copies(c));
    HIPCHK(c, hipEventRecord(c->ev[3], st));
    release_held_camera(c);  // (after a resize that changed the aspect ratio; nothing otherwise)
    return 0;
}

// one denoiser pass on the context's band, enqueued on its stream (vxpt_denoise_pass ids)
// margin (banded chains, band_frame's ghost rows): the pass also computes `margin` rows either side of
// the context's rows (8-aligned, clipped to the frame) -- the rows a later pass of the chain reads there,
// computed here from the same inputs as the neighbour computes them instead of received from it
int run_pass(vxpt_ctx *c, const vxpt_denoise_params *p, int pass, int arg, int arg2, int margin) {
    // a chain composed from single passes on a banded context (bands.py) would drop the two stages silently
    if (const char *sw = prefilter_switch(p))
        if (is_banded(c)) return refuse_prefilter(c, sw);
    DenoiseArgs a{};
    fill_denoise(c, p, a, pass == 0 ? (arg & 1) : 0);
    a.y0 = std::max(0, a.y0 - margin);
    a.y1 = std::min(a.H, a.y1 + margin);
    switch (pass) {
        case 0: HIPCHK(c, firefly_band(a, true, true, c->stream)); break;  // + world positions
        case 2: HIPCHK(c, launch_temporal(a, c->stream)); break;
        case 3: HIPCHK(c, launch_history_fix(a, c->stream)); break;
        case 4: HIPCHK(c, launch_history_clamp(a, c->stream)); break;
        case 5: HIPCHK(c, launch_atrous_smem(a, c->stream)); break;
        case 6: HIPCHK(c, launch_atrous(a, a.ping, a.pong, (unsigned)arg, (unsigned)arg2, false, c->stream)); break;
        case 7: HIPCHK(c, launch_atrous(a, a.pong, a.ping, (unsigned)arg, (unsigned)arg2, false, c->stream)); break;
        case 10: HIPCHK(c, launch_atrous(a, a.ping, a.pong, (unsigned)arg, (unsigned)arg2, true, c->stream)); break;
        case 11: HIPCHK(c, firefly_band(a, false, false, c->stream)); break;
        case 12: HIPCHK(c, launch_frame0_init(a, c->stream)); break;
        case 13: {
            const float4 *src = arg == 1 ? a.ping : (arg == 2 ? a.pong : (arg == 3 ? a.prevIllum : a.illum));
            HIPCHK(c, launch_copy_output(a, src, c->stream));
        } break;
        case 14:  // the end of a chain composed from single passes: as at the end of do_denoise
            HIPCHK(c, history_copies(c));
            release_held_camera(c);
            break;
        case 15:
        case 16:
            if (is_banded(c))
                return refuse_prefilter(c, pass == 15 ? "enable_hit_distance_reconstruction" : "enable_pre_pass");
            if (pass == 15) HIPCHK(c, launch_hitdist(a, c->stream));
            else HIPCHK(c, launch_prepass(a, arg, arg2 == 1, c->stream));
            break;
        default: return fail(c, VXPT_ERR_ARG, "unknown pass");
    }
    return VXPT_OK;
}

}  // namespace vx::host

extern "C" {

int vxpt_trace(vxpt_ctx *c, int32_t it, uint32_t flags) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    const bool accum = (flags & VXPT_TRACE_ACCUMULATE) != 0;
    const int spp = (int)((flags >> 8) & 0xFF);
    if (accum && spp < 1) return fail(c, VXPT_ERR_ARG, "VXPT_TRACE_ACCUMULATE needs the spp in flag bits 8..15");
    c->denoiseInputIsAccum = accum;
    int r = do_trace(c, it, flags, accum, (flags & VXPT_TRACE_ACCUM_FIRST) != 0, accum ? 1.0f / (float)spp : 1.0f);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
    c->timing.trace_ms = ms;
    return VXPT_OK;
}

int vxpt_denoise(vxpt_ctx *c, const vxpt_denoise_params *p, int32_t frameNum, int32_t it) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    int r = do_denoise(c, p, frameNum, it);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
    c->timing.denoise_ms = ms;
    return VXPT_OK;
}

int vxpt_denoise_pass(vxpt_ctx *c, const vxpt_denoise_params *p, int pass, int arg, int arg2) {
    if (!c) return VXPT_ERR_ARG;
    p = denoise_or_yaml(c, p);
    HIPCHK(c, hipSetDevice(c->dev));
    // passes 15 and 16 alone are timed (tools/prefilter_bench.py); every other pass is as it was
    const bool timed = (pass == 15 || pass == 16) && !is_banded(c);
    if (timed) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (int r = run_pass(c, p, pass, arg, arg2)) return r;
    if (timed) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (timed) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        c->timing.denoise_ms = ms;
    }
    return VXPT_OK;
}

int vxpt_render_frame(vxpt_ctx *c, const vxpt_denoise_params *p, int32_t frameNum, int32_t spp) {
    if (!c || spp < 1) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    // refused before anything is enqueued: the context is left as it was
    if (const char *sw = prefilter_switch(denoise_or_yaml(c, p)))
        if (is_banded(c)) return refuse_prefilter(c, sw);
    if (c->comm) {
        std::vector<vxpt_ctx *> cs{c};
        return band_frame(cs, denoise_or_yaml(c, p), frameNum, spp);
    }
    const int it0 = frameNum * spp;
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    for (int s = 0; s < spp; ++s)
        if (int r = do_trace(c, it0 + s, 0, spp > 1, s == 0, 1.0f / (float)spp, s > 0, false, s + 1 == spp)) return r;
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    c->denoiseInputIsAccum = spp > 1;
    int r = do_denoise(c, p, frameNum, it0 + spp);
    if (r) return r;
    HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float t = 0, d = 0, f = 0;
    hipEventElapsedTime(&t, c->ev[6], c->ev[1]);
    hipEventElapsedTime(&d, c->ev[2], c->ev[3]);
    hipEventElapsedTime(&f, c->ev[6], c->ev[7]);
    c->timing.trace_ms = t;
    c->timing.denoise_ms = d;
    c->timing.frame_ms = f;
    return VXPT_OK;
}

int vxpt_render_frames(vxpt_ctx *c, const vxpt_denoise_params *p, int32_t frame0, int32_t nFrames, int32_t spp) {
    if (!c || spp < 1 || nFrames < 1 || frame0 < 0) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    // refused before anything is enqueued: the context is left as it was
    if (const char *sw = prefilter_switch(denoise_or_yaml(c, p)))
        if (is_banded(c)) return refuse_prefilter(c, sw);
    // the frame after a resize that changed the aspect ratio has a previous camera of its own (heldW): it
    // runs unpipelined, since the next frame's first half is planned before this frame's denoiser
    // (the timings are the two runs' combined: means per frame over all nFrames)
    if (c->heldW && nFrames > 1) {
        if (int r = vxpt_render_frames(c, p, frame0, 1, spp)) return r;
        const vxpt_timing first = c->timing;
        if (int r = vxpt_render_frames(c, p, frame0 + 1, nFrames - 1, spp)) return r;
        const float rest = (float)(nFrames - 1), all = (float)nFrames;
        c->timing.trace_ms = (first.trace_ms + c->timing.trace_ms * rest) / all;
        c->timing.denoise_ms = (first.denoise_ms + c->timing.denoise_ms * rest) / all;
        c->timing.frame_ms = (first.frame_ms + c->timing.frame_ms * rest) / all;
        c->timing.host_ms = (first.host_ms + c->timing.host_ms * rest) / all;
        return VXPT_OK;
    }
    const auto hostT0 = std::chrono::steady_clock::now();
    auto hostMs = [&]() {
        return (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - hostT0).count() /
                       nFrames);
    };
    if (c->comm) {  // banded: pipelined like the single-context loop below (band_frame), one sync at the end
        std::vector<vxpt_ctx *> cs{c};
        if (!c->runEv[0])
            for (hipEvent_t &e : c->runEv) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        HIPCHK(c, hipEventRecord(c->runEv[0], c->stream));
        std::vector<PassPlan> pipe;  // the next frame's first pass-halves (band_frame)
        for (int f = 0; f < nFrames; ++f)
            if (int r = band_frame(cs, denoise_or_yaml(c, p), frame0 + f, spp, false, &pipe, f + 1 < nFrames))
                return r;
        HIPCHK(c, hipEventRecord(c->runEv[1], c->stream));
        const float host = hostMs();
        HIPCHK(c, hipStreamSynchronize(c->stream));
        band_timings(cs);  // the last frame's trace / denoiser split
        c->timing.host_ms = host;
        if (c->bst.on)
            if (int r = stat_sync_fold(c)) return r;
        float f = 0;
        hipEventElapsedTime(&f, c->runEv[0], c->runEv[1]);
        c->timing.frame_ms = f / (float)nFrames;
        return VXPT_OK;
    }
    const float scale = 1.0f / (float)spp;
    // events around every denoiser chain: the chains run alone (below), so the frames' trace time is
    // the whole minus their sum.  A chain starts when both the frame's last second half (context
    // stream) and the next frame's first half (its front stream) have finished.  A marker right behind
    // the cross-stream wait is not reliably stamped after the wait (measured 10-40 us early), so an
    // empty one-wave kernel follows the wait and the chain's start marker follows that kernel: the
    // chain is timed from its first kernel's launch, as in a frame call -- the hand-off's own latency
    // (~12 us in a kernel trace: the context stream's first launch after the front stream's last
    // kernel) stays in the frame time, not in the chain's.
    while (c->chainEv.size() < (size_t)3 * nFrames) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        c->chainEv.push_back(e);
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    PassPlan pend;
    bool havePend = false, pendBackQueued = false;
    std::vector<char> frontMarked(nFrames, 0);  // chainEv[3f + 2] recorded in this run
    for (int f = 0; f < nFrames; ++f) {
        const int it0 = (frame0 + f) * spp;
        for (int s = 0; s < spp; ++s) {
            PassPlan pl;
            if (s == 0 && havePend) {
                pl = pend;
                havePend = false;
                if (pendBackQueued) {  // its second half is already behind the previous chain
                    pendBackQueued = false;
                    continue;
                }
            } else if (int r = trace_front(c, it0 + s, 0, spp > 1, s == 0, scale, s > 0, pl, s + 1 == spp)) {
                return r;
            }
            if (int r = trace_back(c, pl, false)) return r;
        }
        if (f + 1 < nFrames) {
            // The next frame's first pass-half runs beside this frame's last second half.  It writes
            // a G-buffer slot that is neither this frame's (the denoiser's input) nor the history
            // the denoiser compares against, the other radiance set, and its own state set; the
            // motion plane it stores is all zeros (static world) like the one the denoiser reads.
            if (int r = trace_front(c, it0 + spp, 0, spp > 1, true, scale, true, pend, spp == 1)) return r;
            havePend = true;
            // the denoiser starts after it, so it runs alone and its timing stays its own.  (Running
            // all of the chain but its firefly stage on a third stream beside the next frame's first
            // pass was measured: 6.02 -> 5.92 ms per frame, but the overlapped chain took ~3x as long
            // and k_restir beside it +0.5 ms; removed)
            // (chains after such a first half measure 0.40 instead of 0.36 ms, every chain kernel 5-10 %
            // slower with the GPU idle beside them; an L2 write-back of the first half's dirty lines
            // before the chain changed nothing -- the frame is still 0.14 ms shorter this way)
            if (!pend.a.primaryOnly && chain_gate(c, spp)) {
                frontMarked[f] = 1;
                HIPCHK(c, hipEventRecord(c->chainEv[3 * f + 2], front_stream(c, pend.set)));
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->frontDone[pend.set], 0));
                HIPCHK(c, launch_stream_mark(c->stream));
                HIPCHK(c, hipEventRecord(c->chainEv[3 * f], c->stream));
            }
        }
        c->denoiseInputIsAccum = spp > 1;
        const bool waited = havePend && !pend.a.primaryOnly && chain_gate(c, spp);
        if (!waited) HIPCHK(c, hipEventRecord(c->chainEv[3 * f], c->stream));
        if (int r = do_denoise(c, p, frame0 + f, it0 + spp)) return r;
        HIPCHK(c, hipEventRecord(c->chainEv[3 * f + 1], c->stream));
        if (havePend) {  // later first halves wait for the denoiser (it reads the old history slot)
            // on the host: the next frame's first second half goes behind the chain on the context
            // stream, then the host waits for the chain before it enqueues any later first half.  A
            // first half parked on a front stream behind a wait for the chain (the device-side gate)
            // slows every kernel launch of the chain (measured: 0.39 ms against 0.36 with the front
            // streams sharing the context stream's hardware queue).
            if (int r = trace_back(c, pend, false)) return r;
            pendBackQueued = true;
            if (chain_gate(c, spp)) HIPCHK(c, hipEventSynchronize(c->chainEv[3 * f + 1]));
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
    c->timing.host_ms = hostMs();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float dsum = 0, f = 0;
    for (int k = 0; k < nFrames; ++k) {
        float a = 0, b = 0, e = 0;
        hipEventElapsedTime(&a, c->ev[6], c->chainEv[3 * k]);
        hipEventElapsedTime(&e, c->ev[6], c->chainEv[3 * k + 1]);
        if (frontMarked[k] && hipEventElapsedTime(&b, c->ev[6], c->chainEv[3 * k + 2]) == hipSuccess)
            a = std::max(a, b);
        dsum += e - a;
    }
    hipEventElapsedTime(&f, c->ev[6], c->ev[7]);
    (void)hipGetLastError();  // a failed timing read must not surface as a later launch's error
    c->timing.trace_ms = (f - dsum) / (float)nFrames;  // per frame, the chains excluded
    c->timing.denoise_ms = dsum / (float)nFrames;        // the mean chain
    c->timing.frame_ms = f / (float)nFrames;
    return VXPT_OK;
}

// ProjectSunToScreen (PostProcessingPipeline.cu:187-206) on the host, like the reference;
// sunLuminance = SkyModel::getAccumulatedSunLuminance, 1 when not positive (:569-571)
static void sun_projection(vxpt_ctx *c, int &on, int &px, int &py, float &u, float &v, float &lum) {
    const V3 uvw = m3_apply(c->cam.worldToUv, normalize(c->sunDir));
    on = 0; px = py = 0; u = v = 0.0f;
    if (uvw.z > 0.0f) {
        const float uu = uvw.x / uvw.z, vv = uvw.y / uvw.z;
        if (!(uu < 0.0f || uu > 1.0f || vv < 0.0f || vv > 1.0f)) {
            on = 1;
            u = uu; v = vv;
            px = std::min(std::max((int)(uu * c->W), 0), c->W - 1);
            py = std::min(std::max((int)(vv * c->H), 0), c->H - 1);
        }
    }
    sky_resolve(c);  // a device-built sky's sun table sum
    lum = c->sunLuminance > 0.0f ? c->sunLuminance : 1.0f;
}

int vxpt_get_sun_projection(vxpt_ctx *c, float out6[6]) {
    if (!c || !out6) return VXPT_ERR_ARG;
    int on, px, py;
    float u, v, lum;
    sun_projection(c, on, px, py, u, v, lum);
    out6[0] = (float)on; out6[1] = (float)px; out6[2] = (float)py; out6[3] = u; out6[4] = v; out6[5] = lum;
    return VXPT_OK;
}

// the post-process buffers, allocated on first use
int post_alloc(vxpt_ctx *c) {
    const size_t n = (size_t)c->maxW * c->maxH;  // the created size: the render size may grow back to it
    if (!c->frame) {
        if (dalloc(c, c->bloomA, n) || dalloc(c, c->bloomB, n) ||
            dalloc(c, c->frame, n) || dalloc(c, c->postHist, kPostHist) || dalloc(c, c->postState, 4))
            return VXPT_ERR_HIP;
        const float init[4] = {0.18f, 1.0f, 0.0f, 0.0f};  // m_currentAvgLuminance (PostProcessingPipeline.cu:433)
        HIPCHK(c, hipMemcpyAsync(c->postState, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->postHist, 0, kPostHist * sizeof(unsigned), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VXPT_OK;
}

// the context's post-process arguments
int post_args(vxpt_ctx *c, const vxpt_post_params *pp, float dtMs, PostArgs &a) {
    if (!pp) pp = &c->yamlPost;
    if (int r = post_alloc(c)) return r;
    a = PostArgs{};
    a.W = c->W; a.H = c->H;
    a.y0 = c->rowBegin; a.y1 = c->rowEnd;
    a.p = {pp->manual_exposure, pp->tone_mapping_curve, pp->white_point, pp->contrast, pp->saturation, pp->lift,
           pp->gain, pp->enable_bloom, pp->bloom_threshold, pp->bloom_intensity, pp->bloom_radius,
           pp->enable_auto_exposure, pp->exposure_speed, pp->exposure_min, pp->exposure_max,
           pp->exposure_compensation, pp->histogram_min_percent, pp->histogram_max_percent, pp->target_luminance,
           pp->enable_vignette, pp->vignette_strength, pp->vignette_radius, pp->vignette_smoothness,
           pp->enable_lens_flare, pp->lens_flare_intensity, pp->lens_flare_ghost_spacing,
           pp->lens_flare_ghost_count, pp->lens_flare_halo_radius, pp->lens_flare_sun_size,
           pp->lens_flare_distortion, pp->draw_crosshair};
    a.input = c->output;
    a.bloomA = c->bloomA; a.bloomB = c->bloomB; a.frame = c->frame;
    a.depth = c->gb[c->last].depth;
    a.hist = c->postHist;
    a.state = c->postState;
    a.dtMs = dtMs;
    sun_projection(c, a.sunOnScreen, a.sunPx, a.sunPy, a.sunU, a.sunV, a.sunLuminance);
    return VXPT_OK;
}

int vxpt_postprocess(vxpt_ctx *c, const vxpt_post_params *pp, float dtMs) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    if (c->comm && c->nranks > 1) {
        std::vector<vxpt_ctx *> cs{c};
        return band_post(cs, pp, dtMs);
    }
    PostArgs a;
    if (int r = post_args(c, pp, dtMs, a)) return r;
    HIPCHK(c, launch_postprocess(a, c->stream));
    return VXPT_OK;
}

namespace {
bool upscale_args_ok(int w, int h, int ow, int oh, int mode, float sharpness) {
    return w > 0 && h > 0 && ow >= w && oh >= h && mode >= VXPT_UPSCALE_BICUBIC && mode <= VXPT_UPSCALE_EASU_SHARPEN &&
           sharpness >= 0.0f && sharpness <= 1.0f;  // a NaN fails both compares
}
}  // namespace

int vxpt_upscale(vxpt_ctx *c, int outW, int outH, int mode, float sharpness) {
    if (!c) return VXPT_ERR_ARG;
    if (!upscale_args_ok(c->W, c->H, outW, outH, mode, sharpness))
        return fail(c, VXPT_ERR_ARG, "vxpt_upscale: output smaller than the frame, unknown mode or sharpness outside [0, 1]");
    if (!c->frame) return fail(c, VXPT_ERR_STATE, "vxpt_upscale: no frame (vxpt_postprocess or vxpt_upload first)");
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t px = (size_t)outW * outH, n = mode == VXPT_UPSCALE_EASU_SHARPEN ? 2 * px : px;
    if (n > c->upscaledCap) {
        if (c->upscaled) {  // earlier calls may still read it
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), (void *)c->upscaled));
            HIPCHK(c, hipFree(c->upscaled));
            c->upscaled = nullptr;
            c->upscaledCap = 0;
            c->upW = c->upH = 0;
        }
        if (dalloc(c, c->upscaled, n)) return VXPT_ERR_HIP;
        c->upscaledCap = n;
    }
    for (hipEvent_t &e : c->upEv)
        if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    HIPCHK(c, hipEventRecord(c->upEv[0], c->stream));
    HIPCHK(c, launch_upscale(c->frame, c->W, c->H, c->upscaled, c->upscaled + px, outW, outH, mode, sharpness, c->stream));
    HIPCHK(c, hipEventRecord(c->upEv[1], c->stream));
    c->upW = outW;
    c->upH = outH;
    return VXPT_OK;
}

int vxpt_upscale_info(vxpt_ctx *c, int *outW, int *outH, float *ms) {
    if (!c) return VXPT_ERR_ARG;
    if (c->upW <= 0) return fail(c, VXPT_ERR_STATE, "vxpt_upscale_info: no vxpt_upscale yet");
    if (outW) *outW = c->upW;
    if (outH) *outH = c->upH;
    if (ms) {
        HIPCHK(c, hipSetDevice(c->dev));
        HIPCHK(c, hipEventSynchronize(c->upEv[1]));
        HIPCHK(c, hipEventElapsedTime(ms, c->upEv[0], c->upEv[1]));
    }
    return VXPT_OK;
}

int vxpt_upscale_host(const float *in, int w, int h, float *out, int outW, int outH, int mode, float sharpness) {
    if (!in || !out || !upscale_args_ok(w, h, outW, outH, mode, sharpness)) return VXPT_ERR_ARG;
    upscale_host(in, w, h, out, outW, outH, mode, sharpness);
    return VXPT_OK;
}

int vxpt_prefilter_host(int stage, int w, int h, const vxpt_camera *cam, int32_t iterationIndex, const float *illum,
                        const float *depth, const float *normalRough, const float *material, float *out,
                        int32_t *tapXY) {
    if ((stage != 0 && stage != 1) || w < 1 || h < 1 || !cam || !illum || !depth || !normalRough || !material || !out ||
        illum == out)
        return VXPT_ERR_ARG;
    prefilter_host(stage, make_camera(w, h, *cam, nullptr, nullptr), w, h, iterationIndex, illum, depth, normalRough,
                   material, out, stage == 1 ? tapXY : nullptr);
    return VXPT_OK;
}

int vxpt_debug_clamp_decisions(vxpt_ctx *c, int on) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (on && !c->clampDbg)  // kept until the context goes (zero-filled)
        if (int r = dalloc(c, c->clampDbg, (size_t)c->maxW * c->maxH)) return r;
    c->clampDbgOn = on != 0;
    return VXPT_OK;
}

}  // extern "C"
