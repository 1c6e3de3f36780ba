// vxpt -- host runtime, dynamic resolution: the render size changed between frames with the histories
// resampled to the new size (Backend::dynamicResolution, Backend.cpp:191-232), the
// resample's host twin and the reference's frame-time controller as a pure function.
#include <cmath>
#include <utility>
#include <vector>

#include "host_ctx.hpp"
#include "resize.hpp"

namespace {

// The planes of one record size: one launch per table of kResizePlanes (a full table starts the next)
struct Batch {
    std::vector<ResizePlanes> tables;
    void add(const void *src, void *dst) {
        if (tables.empty() || tables.back().n == kResizePlanes) tables.push_back(ResizePlanes{});
        ResizePlanes &p = tables.back();
        p.src[p.n] = src;
        p.dst[p.n] = dst;
        ++p.n;
    }
    hipError_t launch(int bytesPerPixel, int oldW, int oldH, int newW, int newH, hipStream_t st) const {
        for (const ResizePlanes &p : tables)
            if (hipError_t e = launch_resize(p, bytesPerPixel, oldW, oldH, newW, newH, st)) return e;
        return hipSuccess;
    }
};

// the shadows of the planes outside the G-buffer ring, at the created size
int shadow_alloc(vxpt_ctx *c) {
    if (c->shRes) return 0;
    const size_t n = (size_t)c->maxW * c->maxH;
    if (dalloc(c, c->shPrevIllum, n) || dalloc(c, c->shPrevFast, n) || dalloc(c, c->shMotion, n) ||
        dalloc(c, c->shHistLen, n) || dalloc(c, c->shPrevHistLen, n) || dalloc(c, c->shRes, 2 * n))
        return VXPT_ERR_HIP;
    for (hipEvent_t &e : c->rzEv) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    return 0;
}

// Every buffer a later frame reads before it writes it, from oldW x oldH to the context's (new) size.
// Nothing is in flight (the caller waited), so a destination may be any plane that holds nothing a later
// frame reads: the shadows, and the ring's slots without a role.
int resample(vxpt_ctx *c, int oldW, int oldH) {
    if (int r = shadow_alloc(c)) return r;
    Batch b4, b16, b20, b32;
    const size_t oldN = (size_t)oldW * oldH, newN = (size_t)c->W * c->H;
    // the ring: the slots with a role -- the last pass's (the next pass's temporal taps; the current planes),
    // the denoiser's history, the slot the last pass read (the PREV_* planes of vxpt_readback) -- move to
    // slots without one
    int moved[6];
    bool taken[6] = {};
    for (int k = 0; k < 6; ++k) moved[k] = -1;
    for (int live : {c->last, c->hist, c->tracePrev}) taken[live] = true;
    int to = 0;
    for (int live : {c->last, c->hist, c->tracePrev}) {
        if (moved[live] >= 0) continue;
        while (taken[to]) ++to;  // at most 3 of the 6 slots are taken by roles
        taken[to] = true;
        moved[live] = to;
        const GSlot &s = c->gb[live];
        GSlot &d = c->gb[to];
        b16.add(s.normalRough, d.normalRough);
        b16.add(s.geoNormalThin, d.geoNormalThin);
        b16.add(s.albedo, d.albedo);
        b16.add(s.matParam, d.matParam);
        b4.add(s.depth, d.depth);
        b4.add(s.material, d.material);
        b32.add(s.rec, d.rec);
        d.recStale = s.recStale;
    }
    b16.add(c->prevIllum, c->shPrevIllum);
    b16.add(c->prevFast, c->shPrevFast);
    if (!c->motionZero) b16.add(c->motion, c->shMotion);  // (the static world's plane holds zeros at any size)
    b4.add(c->histLen, c->shHistLen);
    b4.add(c->prevHistLen, c->shPrevHistLen);
    // both parities: the second one starts at the size's pixel count
    b20.add(c->res, c->shRes);
    b20.add(c->res + oldN, c->shRes + newN);
    HIPCHK(c, hipEventRecord(c->rzEv[0], c->stream));
    HIPCHK(c, b4.launch(4, oldW, oldH, c->W, c->H, c->stream));
    HIPCHK(c, b16.launch(16, oldW, oldH, c->W, c->H, c->stream));
    HIPCHK(c, b32.launch(32, oldW, oldH, c->W, c->H, c->stream));
    HIPCHK(c, b20.launch(20, oldW, oldH, c->W, c->H, c->stream));
    HIPCHK(c, hipEventRecord(c->rzEv[1], c->stream));
    c->rzTimed = true;
    // the destinations become the buffers
    c->last = moved[c->last];
    c->hist = moved[c->hist];
    c->tracePrev = moved[c->tracePrev];
    c->tracePrev2 = c->tracePrev;  // nothing in flight reads the older slots
    c->histOld = c->hist;
    std::swap(c->prevIllum, c->shPrevIllum);
    std::swap(c->prevFast, c->shPrevFast);
    if (!c->motionZero) std::swap(c->motion, c->shMotion);
    std::swap(c->histLen, c->shHistLen);
    std::swap(c->prevHistLen, c->shPrevHistLen);
    std::swap(c->res, c->shRes);
    return 0;
}

}  // namespace

extern "C" {

int vxpt_set_render_size(vxpt_ctx *c, int w, int h) {
    if (!c) return VXPT_ERR_ARG;
    if (w < 1 || h < 1 || w > c->maxW || h > c->maxH || c->maxW > resize::kResizeMaxDim || c->maxH > resize::kResizeMaxDim)
        return fail(c, VXPT_ERR_ARG, "vxpt_set_render_size: the size must lie between 1 x 1 and the created size");
    if (is_banded(c))
        return fail(c, VXPT_ERR_STATE, "vxpt_set_render_size is not supported on banded contexts (a row range, a band "
                                       "communicator or linked contexts)");
    if (w == c->W && h == c->H) return VXPT_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    // behind everything in flight: the resample reads what the streams still write, and its
    // destinations are planes they may still read
    for (hipStream_t fs : c->frontStreams) HIPCHK(c, hipStreamSynchronize(fs));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int oldW = c->W, oldH = c->H;
    c->W = w;
    c->H = h;
    c->rowBegin = 0;
    c->rowEnd = h;
    const bool history = c->passCount > 0 || c->hostWrote;
    if (history) {
        if (int r = resample(c, oldW, oldH)) {
            c->W = oldW; c->H = oldH; c->rowEnd = oldH;
            return r;
        }
        // the history now holds the old size's view: when that has another aspect ratio (the vertical field
        // of view follows it) the previous camera keeps it for one frame.  A second resize before that
        // frame leaves the first one's size held: the history is still that view
        if (!c->heldW && (float)oldH / (float)oldW != (float)h / (float)w) { c->heldW = oldW; c->heldH = oldH; }
    }
    if (c->camSrc.set) c->cam = make_camera_src(w, h, c->camSrc);
    if (c->prevCamSrc.set) c->prevCam = history_camera(c, c->prevCamSrc);
    return VXPT_OK;
}

int vxpt_get_render_size(vxpt_ctx *c, int *w, int *h, int *max_w, int *max_h) {
    if (!c) return VXPT_ERR_ARG;
    if (w) *w = c->W;
    if (h) *h = c->H;
    if (max_w) *max_w = c->maxW;
    if (max_h) *max_h = c->maxH;
    return VXPT_OK;
}

int vxpt_render_size_ms(vxpt_ctx *c, float *ms) {
    if (!c || !ms) return VXPT_ERR_ARG;
    if (!c->rzTimed) return fail(c, VXPT_ERR_STATE, "vxpt_render_size_ms: no resample yet");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipEventSynchronize(c->rzEv[1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->rzEv[0], c->rzEv[1]));
    return VXPT_OK;
}

int vxpt_resize_host(const void *src, int old_w, int old_h, void *dst, int new_w, int new_h, int bytes_per_pixel) {
    const int lim = resize::kResizeMaxDim;
    if (!src || !dst || old_w < 1 || old_h < 1 || new_w < 1 || new_h < 1 || old_w > lim || old_h > lim || new_w > lim ||
        new_h > lim || !resize::bpp_ok(bytes_per_pixel))
        return VXPT_ERR_ARG;
    resize::resize_host(src, dst, resize::Map{old_w, old_h, new_w, new_h}, bytes_per_pixel);
    return VXPT_OK;
}

// Backend.cpp:209-222, statement for statement (renderWidth *= ratio converts the float product back to int)
int vxpt_dynres_next_width(int cur_w, float frame_ms, float target_fps, int min_w, int max_w, int *next_w, int *next_h) {
    if (!next_w || cur_w < 1 || !(frame_ms > 0.0f) || !(target_fps > 0.0f) || min_w < 1 || min_w > max_w)
        return VXPT_ERR_ARG;
    int w = cur_w;
    const float high = 1000.0f / (target_fps - 2.0f), low = 1000.0f / (target_fps + 2.0f);
    if (high < frame_ms || low > frame_ms) {
        float ratio = (1000.0f / target_fps) / frame_ms;
        ratio = sqrtf(ratio);
        const float scaled = (float)w * ratio;
        w = scaled < 1073741824.0f ? (int)scaled : 1073741824;  // (converting a float past INT_MAX is undefined)
    }
    w = w + ((w % 16 < 8) ? (-w % 16) : (16 - w % 16));
    w = w < min_w ? min_w : (w > max_w ? max_w : w);
    *next_w = w;
    if (next_h) *next_h = (w / 16) * 9;
    return VXPT_OK;
}

}  // extern "C"
