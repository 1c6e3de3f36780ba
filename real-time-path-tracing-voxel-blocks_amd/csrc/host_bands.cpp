// vxpt -- host runtime, the band partition (multi-GPU): band rows and halo planning, the halo
// exchange over RCCL or between linked contexts, statistics, the banded frame and post-process,
// the gather.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "host_ctx.hpp"

namespace {

// ---------------------------------------------------------------- band partition
// The multi-GPU schedule of one frame (bands.py restates it for
// the CPU tests): every rank traces and denoises its 8-row-aligned band into
// full-frame buffers, and every pass that reads a neighbourhood is preceded by
// an exchange of exactly the rows it reads outside the band, with the band
// neighbours r +/- 1.  Rows are contiguous in every plane, so a halo is one
// ncclSend / ncclRecv per plane and neighbour, grouped, enqueued on the
// context stream behind the kernels that produced the rows -- no packing, no
// host synchronisation.
constexpr int kTraceHalo = 72;  // ReSTIR temporal taps: 64-pixel disk + reprojection (Restir.h:348-381)
// The next pass's temporal taps read only the previous pass's tap records (GBuf::rec) and reservoirs,
// so a pass hands its neighbours those two, 52 B/px, at the trace depth; the G-buffer planes are
// read by the denoiser alone (after the frame's last pass, within kDenoiseRows of the band: the
// world positions of k_firefly at kWposHalo, the history fix's taps at 34) and by the next frame's
// temporal accumulation as its history (histRows), so they travel once per frame.
const int kGbufPlanes[] = {VXPT_BUF_DEPTH, VXPT_BUF_NORMAL_ROUGH, VXPT_BUF_GEO_NORMAL_THIN,
                           VXPT_BUF_ALBEDO, VXPT_BUF_MATERIAL, VXPT_BUF_MAT_PARAM};
// a host-side write to a G-buffer plane leaves the slots' tap records stale (rebuilt before the next
// trace reads them)
bool is_gbuf_plane(int which) { return (which >= VXPT_BUF_DEPTH && which <= VXPT_BUF_MAT_PARAM) ||
                                       (which >= VXPT_BUF_PREV_NORMAL_ROUGH && which <= VXPT_BUF_PREV_MATERIAL); }

const int kHistoryBufs[] = {VXPT_BUF_PREV_ILLUM, VXPT_BUF_PREV_FAST, VXPT_BUF_PREV_HIST_LEN};

void band_rows(int H, int world, int rank, int &y0, int &y1) {
    const int per = (H + 8 * world - 1) / (8 * world) * 8;
    y0 = std::min(H, rank * per);
    y1 = std::min(H, y0 + per);
}

// the equal bands' boundaries: band r = rows [s[r], s[r + 1])
std::vector<int> equal_splits(int H, int world) {
    std::vector<int> s(world + 1, 0);
    for (int r = 0; r < world; ++r) band_rows(H, world, r, s[r], s[r + 1]);
    return s;
}

// an uneven partition (vxpt_band_comm_init_rows): 0 = s[0] < s[1] < ... < s[n] = H, inner
// boundaries 8-aligned (vxpt_set_band), every band at least the ReSTIR halo tall when n > 1
bool splits_valid(const int32_t *s, int n, int H, int minRows) {
    if (!s || n < 1 || s[0] != 0 || s[n] != H) return false;
    for (int k = 0; k < n; ++k)
        if (s[k + 1] - s[k] < (n > 1 ? minRows : 1) || (k > 0 && (s[k] & 7))) return false;
    return true;
}

struct Halo { int peer, sy, sn, ry, rn; };
// rows rank sends to / receives from each band neighbour of the partition s (both sides of a
// border move min(rows, the two band heights) rows)
std::vector<Halo> halo_plan(const std::vector<int> &s, int rank, int rows) {
    std::vector<Halo> plan;
    const int world = (int)s.size() - 1;
    const int y0 = s[rank], y1 = s[rank + 1];
    if (rank > 0) {
        const int n = std::min(rows, std::min(y1 - y0, s[rank] - s[rank - 1]));
        plan.push_back({rank - 1, y0, n, y0 - n, n});
    }
    if (rank < world - 1) {
        const int n = std::min(rows, std::min(y1 - y0, s[rank + 2] - s[rank + 1]));
        plan.push_back({rank + 1, y1 - n, n, y1, n});
    }
    return plan;
}

// the context's partition: its row_splits, or the equal bands
std::vector<int> splits_of(const vxpt_ctx *c) {
    return (int)c->splits.size() == c->nranks + 1 ? c->splits : equal_splits(c->H, c->nranks);
}

// Halo depths of a banded frame whose camera moved between passes (cur vs prev).  A band's
// pixels reproject to rows prevCam.dir_to_uv(hit - prevCam.pos).y * H: the ReSTIR temporal taps
// read the previous pass's G-buffer and reservoirs within 64 rows of that row (Restir.h:348-381,
// truncated row), the temporal accumulation its histories within its bicubic footprint (-1..+2
// around floor(row - 0.5), TemporalAccumulation.h:29-215).  For a rotation the reprojection does
// not depend on depth: the extreme rows over the band come from the pixel corners on the band's
// first and last row boundaries (all columns) plus a 33-column grid over every row; 2 rows of
// margin cover host/device rounding.  A translation t makes a pixel's row depend on its hit
// distance d: row(d) = (d a.y + b.y) / (d a.z + b.z) with a = worldToUv dir, b = worldToUv t, a
// Moebius map of d, monotone on [nearDepth, inf) while its denominator stays positive there -- so
// with a lower bound nearDepth on every primary hit's distance the extremes are the rows at
// nearDepth and at infinity (the rotation's), sampled on a 129-column grid.  Without such a bound
// (nearDepth <= 0) a translated camera is refused; so is a point behind the previous camera or a
// halo deeper than a neighbouring band (the plan only reaches ranks r +/- 1).  An unmoved camera
// keeps the static depths (72 / 2).
bool band_halo_rows(const CamDev &cam, const CamDev &pc, int W, int H, const std::vector<int> &splits,
                    int &traceRows, int &histRows, std::string &err, float nearDepth = 0.0f) {
    const int world = (int)splits.size() - 1;
    traceRows = kTraceHalo;
    histRows = 2;
    if (world <= 1) return true;
    if (std::memcmp(&cam, &pc, sizeof(CamDev)) == 0) return true;
    const V3 t = cam.pos - pc.pos;
    const bool moved = t.x != 0.0f || t.y != 0.0f || t.z != 0.0f;
    if (moved && !(nearDepth > 0.0f)) {
        err = "banded frames need a camera that does not translate between passes, or a lower bound on the "
              "primary hits' distance (depth-dependent reprojection)";
        return false;
    }
    const V3 b = m3_apply(pc.worldToUv, t);
    const int cols = moved ? 128 : 32;
    int minBand = H;
    float reach = 0.0f;  // rows beyond its band any band pixel reprojects to
    for (int r = 0; r < world; ++r) {
        const int y0 = splits[r], y1 = splits[r + 1];
        if (y1 <= y0) continue;
        minBand = std::min(minBand, y1 - y0);
        float lo = 1e30f, hi = -1e30f;
        bool behind = false;
        auto sample = [&](float u, float v) {
            const V3 d = cam.uv_to_dir(V2(u, v));
            const V3 n = m3_apply(pc.worldToUv, d);
            if (!(n.z > 0.0f)) { behind = true; return; }
            const float py = n.y / n.z * (float)H;
            lo = std::min(lo, py);
            hi = std::max(hi, py);
            if (moved) {  // the hit at the nearest distance
                const V3 m = n * nearDepth + b;
                if (!(m.z > 0.0f)) { behind = true; return; }
                const float pm = m.y / m.z * (float)H;
                lo = std::min(lo, pm);
                hi = std::max(hi, pm);
            }
        };
        for (int x = 0; x <= W; ++x) {
            sample((float)x / (float)W, (float)y0 / (float)H);
            sample((float)x / (float)W, (float)y1 / (float)H);
        }
        for (int y = y0; y <= y1; ++y)
            for (int k = 0; k <= cols; ++k) sample((float)k / (float)cols, (float)y / (float)H);
        if (behind) {
            err = "the camera moved so far that part of a band lies behind the previous camera";
            return false;
        }
        if (r > 0) reach = std::max(reach, (float)y0 - lo);
        if (r < world - 1) reach = std::max(reach, hi - (float)y1);
    }
    const int d = (int)std::ceil(std::max(reach, 0.0f)) + 2;
    traceRows = std::max(kTraceHalo, 64 + d + 1);
    histRows = std::max(2, d + 2);
    if (traceRows > minBand) {
        err = "the camera moved " + std::to_string(d) + " rows between passes: a " + std::to_string(traceRows) +
              "-row halo exceeds the " + std::to_string(minBand) + "-row bands";
        return false;
    }
    return true;
}

char *buffer_rows(vxpt_ctx *c, int which, int y, size_t &rowBytes) {
    void *p, *mirror;
    size_t n;
    buffer_ptr(c, which, p, n, false, &mirror);
    rowBytes = n / (size_t)c->H;
    return static_cast<char *>(p) + (size_t)y * rowBytes;
}

// Halo exchange of `bufs` over `rows` rows for every context of the frame
// (one with RCCL, all of this process's bands when linked).
// With overlap (RCCL only) the exchange runs on the context's exchange stream
// after the rows' producer and the next trace pass's temporal-reuse kernel waits
// for it (do_trace); the trace passes touch neither the sent rows nor the
// received ones before that kernel (they write the other G-buffer slot and
// reservoir parity).
// several buffers with their own halo depths in one group (one RCCL launch, one sync point)
// after (RCCL, overlap): the exchange starts once that event has completed instead of behind the
// context stream's work so far (the tap records: after the producing pass's first half)
int exchange_set(std::vector<vxpt_ctx *> &cs, const std::vector<std::pair<int, int>> &bufRows, bool overlap = false,
                 hipEvent_t after = nullptr);

int exchange(std::vector<vxpt_ctx *> &cs, const std::vector<int> &bufs, int rows, bool overlap = false) {
    std::vector<std::pair<int, int>> br;
    for (int b : bufs) br.emplace_back(b, rows);
    return exchange_set(cs, br, overlap);
}

#define BANDCHK_(expr)                  \
    do {                                \
        if (int r_ = (expr)) return r_; \
    } while (0)
// a vxpt_band_stats timing event recorded on st (collection on), its pool index
int stat_mark(vxpt_ctx *c, hipStream_t st, size_t &idx) {
    auto &b = c->bst;
    if (b.used == b.pool.size()) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        b.pool.push_back(e);
    }
    idx = b.used++;
    HIPCHK(c, hipEventRecord(b.pool[idx], st));
    return 0;
}
// the collected spans' times into the running totals, their events back to the pool (every span's
// events have completed: the caller synchronised the context and exchange streams)
constexpr size_t kStatPoolFold = 512;
int stat_fold(vxpt_ctx *c) {
    auto &b = c->bst;
    for (const auto &sp : b.spans) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, b.pool[sp.e0], b.pool[sp.e1]));
        b.ms[sp.kind] += ms;
    }
    b.spans.clear();
    b.used = 0;
    return VXPT_OK;
}

// the bytes a halo plan entry sends, to the neighbour above (peer < rank) or below
void stat_bytes(vxpt_ctx *c, const Halo &h, size_t rowBytes) {
    (h.peer < c->rank ? c->bst.up : c->bst.down) += (double)h.sn * (double)rowBytes;
}

int exchange_set(std::vector<vxpt_ctx *> &cs, const std::vector<std::pair<int, int>> &bufRows, bool overlap,
                 hipEvent_t after) {
    if (cs.size() == 1 && cs[0]->comm) {
        vxpt_ctx *c = cs[0];
        hipStream_t st = c->stream;
        if (overlap) {
            if (!after) {
                HIPCHK(c, hipEventRecord(c->haloReady, c->stream));
                after = c->haloReady;
            }
            HIPCHK(c, hipStreamWaitEvent(c->commStream, after, 0));
            if (c->exDoneRec) HIPCHK(c, hipStreamWaitEvent(c->commStream, c->exDone, 0));
            st = c->commStream;
        } else if (c->haloPending) {
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->haloDone, 0));
        }
        size_t m0 = 0, m1 = 0;
        if (c->bst.on) BANDCHK_(stat_mark(c, st, m0));
        if (ncclGroupStart() != ncclSuccess) return fail(c, VXPT_ERR_HIP, "ncclGroupStart");
        ncclResult_t rc = ncclSuccess;
        for (const auto &br : bufRows)
            for (const Halo &h : halo_plan(splits_of(c), c->rank, br.second)) {
                const int b = br.first;
                size_t rb;
                char *send = buffer_rows(c, b, h.sy, rb);
                char *recv = buffer_rows(c, b, h.ry, rb);
                if (rc == ncclSuccess) rc = ncclSend(send, (size_t)h.sn * rb, ncclUint8, h.peer, c->comm, st);
                if (rc == ncclSuccess) rc = ncclRecv(recv, (size_t)h.rn * rb, ncclUint8, h.peer, c->comm, st);
                if (c->bst.on) stat_bytes(c, h, rb);
            }
        const ncclResult_t re = ncclGroupEnd();  // closes the group whatever failed inside it
        if (rc != ncclSuccess)
            return fail(c, VXPT_ERR_HIP, std::string("ncclSend/ncclRecv (halo exchange): ") + ncclGetErrorString(rc));
        if (re != ncclSuccess)
            return fail(c, VXPT_ERR_HIP, std::string("ncclGroupEnd (halo exchange): ") + ncclGetErrorString(re));
        if (c->bst.on) {
            BANDCHK_(stat_mark(c, st, m1));
            c->bst.spans.push_back({m0, m1, overlap ? 1 : 0});
            ++c->bst.groups;
            if (!overlap) ++c->bst.groupsOrdered;
        }
        if (overlap) {
            HIPCHK(c, hipEventRecord(c->haloDone, c->commStream));
            c->haloPending = true;
        } else {
            HIPCHK(c, hipEventRecord(c->exDone, c->stream));
            c->exDoneRec = true;
        }
        return VXPT_OK;
    }
    // linked contexts of one process: device copies from each neighbour's own rows
    // (never written by an exchange), after every band finished the producing pass
    for (vxpt_ctx *c : cs) HIPCHK(c, hipStreamSynchronize(c->stream));
    for (vxpt_ctx *c : cs) {
        size_t m0 = 0, m1 = 0;
        if (c->bst.on) BANDCHK_(stat_mark(c, c->stream, m0));
        for (const auto &br : bufRows)
            for (const Halo &h : halo_plan(splits_of(c), c->rank, br.second)) {
                const int b = br.first;
                size_t rb;
                char *dst = buffer_rows(c, b, h.ry, rb);
                const char *src = buffer_rows(cs[h.peer], b, h.ry, rb);
                HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)h.rn * rb, hipMemcpyDeviceToDevice, c->stream));
                // this band's rows the neighbour copies: what an RCCL rank sends
                if (c->bst.on) stat_bytes(c, h, rb);
            }
        if (c->bst.on) {
            BANDCHK_(stat_mark(c, c->stream, m1));
            c->bst.spans.push_back({m0, m1, 0});
            ++c->bst.groups;
            ++c->bst.groupsOrdered;
        }
    }
    for (vxpt_ctx *c : cs) HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

int atrous_rows(int step) { return step + (step > 4 ? step / 4 : 0); }  // Atrous.h:79-84 jitter above step 4

#define BANDCHK(expr)              \
    do {                           \
        if (int r_ = (expr)) return r_; \
    } while (0)
#define FOR_BANDS(expr)                 \
    do {                                \
        for (vxpt_ctx *c : cs) BANDCHK(expr); \
    } while (0)

}  // namespace

namespace vx::host {

void gbuf_written(vxpt_ctx *c, int which) {
    c->hostWrote = true;
    if (which == VXPT_BUF_MOTION) c->motionZero = false;
    if (is_gbuf_plane(which))
        for (GSlot &g : c->gb) g.recStale = true;
}

int stat_sync_fold(vxpt_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->commStream) HIPCHK(c, hipStreamSynchronize(c->commStream));
    return stat_fold(c);
}

// One banded OfflineBackend::renderFrame over cs (vxpt_render_frame's order).
// the last banded frame's timings (its events complete: after a sync of the context streams)
void band_timings(std::vector<vxpt_ctx *> &cs) {
    for (vxpt_ctx *c : cs) {
        float t = 0, d = 0, f = 0;
        hipEventElapsedTime(&t, c->ev[6], c->ev[1]);
        hipEventElapsedTime(&d, c->ev[2], c->ev[3]);
        hipEventElapsedTime(&f, c->ev[6], c->ev[7]);
        c->timing.trace_ms = t;   // the band's trace passes and their halo exchanges
        c->timing.denoise_ms = d; // the band's denoiser passes and their halo exchanges
        c->timing.frame_ms = f;
    }
}

// sync = false (a run of frames, vxpt_render_frames): enqueue the frame and return, so that the host
// enqueues the next frame while this one runs; the caller syncs after the last.
// pipe (the pipelined run, vxpt_render_frames' order for bands): when it holds plans, they are this
// frame's first pass-halves, enqueued by the previous frame's call beside its last second half, and
// this call opens with their second halves; with pipeNext this call leaves the next frame's first
// pass-halves in it (their first halves run beside this frame's last second half and its exchange,
// the denoiser chain after them), and the next call gates its later first halves on the host behind
// this frame's chain (vxpt_render_frames' host gate: no front stream parked behind a wait for it).
int band_frame(std::vector<vxpt_ctx *> &cs, const vxpt_denoise_params *p, int frame, int spp, bool sync,
               std::vector<PassPlan> *pipe, bool pipeNext) {
    if (const char *sw = prefilter_switch(p)) return refuse_prefilter(cs[0], sw);
    const int it0 = frame * spp;
    // halo depths for this frame's camera motion; the previous frame exchanged its last pass's
    // rows and the histories for its own camera: top them up before the first pass reads them
    int traceRows = kTraceHalo, histRows = 2;
    {
        vxpt_ctx *c0 = cs[0];
        std::string err;
        // a translated camera: the nearest surface bounds every primary hit's distance
        const bool moved = c0->cam.pos.x != c0->prevCam.pos.x || c0->cam.pos.y != c0->prevCam.pos.y ||
                           c0->cam.pos.z != c0->prevCam.pos.z;
        float nearDepth = 0.0f;
        bool reused = false;
        auto search = [&]() {
            nearDepth = nearest_surface(c0, c0->cam.pos);
            c0->nearPos = c0->cam.pos;
            c0->nearDist = nearDepth;
            c0->nearVersion = c0->worldVersion;
        };
        if (moved) {
            const V3 dp = c0->cam.pos - c0->nearPos;
            const float reuse = c0->nearDist - std::sqrt(dp.x * dp.x + dp.y * dp.y + dp.z * dp.z);
            reused = c0->nearVersion == c0->worldVersion && reuse >= 0.75f * c0->nearDist && reuse > 0.0f;
            if (reused) nearDepth = reuse;
            else search();
        }
        bool ok = band_halo_rows(c0->cam, c0->prevCam, c0->W, c0->H, splits_of(c0), traceRows, histRows, err, nearDepth);
        if (!ok && reused) {  // the reused bound is looser than a fresh search: search before refusing
            search();
            ok = band_halo_rows(c0->cam, c0->prevCam, c0->W, c0->H, splits_of(c0), traceRows, histRows, err, nearDepth);
        }
        if (!ok) return fail(c0, VXPT_ERR_STATE, err.c_str());
    }
    // the G-buffer planes' depth: the denoiser's reads, or the next temporal accumulation's history
    const int planeRows = std::max(kDenoiseRows, histRows);
    if (frame > 0 && (traceRows > cs[0]->haloTraceRows || histRows > cs[0]->haloHistRows ||
                      planeRows > cs[0]->haloPlaneRows)) {
        std::vector<std::pair<int, int>> br;
        br.emplace_back(VXPT_BUF_TAP_RECORD, traceRows);
        br.emplace_back(((it0 - 1) & 1) ? VXPT_BUF_RES_ODD : VXPT_BUF_RES_EVEN, traceRows);
        for (int b : kGbufPlanes) br.emplace_back(b, planeRows);
        for (int b : kHistoryBufs) br.emplace_back(b, histRows);
        BANDCHK(exchange_set(cs, br, false));
    }
    for (vxpt_ctx *c : cs) {
        c->haloTraceRows = traceRows;
        c->haloHistRows = histRows;
        c->haloPlaneRows = planeRows;
    }
    for (vxpt_ctx *c : cs)  // no span of this frame is open yet: a full pool is folded here
        if (c->bst.on && c->bst.used >= kStatPoolFold) BANDCHK(stat_sync_fold(c));
    for (vxpt_ctx *c : cs) HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    std::vector<size_t> mk(cs.size() * 3, 0);  // vxpt_band_stats: trace start, trace end, denoiser end
    for (size_t k = 0; k < cs.size(); ++k)
        if (cs[k]->bst.on) BANDCHK(stat_mark(cs[k], cs[k]->stream, mk[3 * k]));
    const bool piped = pipe && pipe->size() == cs.size();
    for (int s = 0; s < spp; ++s) {
        if (s == 0 && piped) {
            for (size_t k = 0; k < cs.size(); ++k) BANDCHK(trace_back(cs[k], (*pipe)[k], false));
            pipe->clear();
            // the later first halves are enqueued once the previous frame's chain has finished (chain_gate)
            for (vxpt_ctx *c : cs)
                if (chain_gate(c, spp)) HIPCHK(c, hipEventSynchronize(c->ev[7]));
        } else {
            FOR_BANDS(do_trace(c, it0 + s, 0, spp > 1, s == 0, 1.0f / (float)spp, s > 0, false, s + 1 == spp));
        }
        if (s + 1 == spp && pipe && pipeNext) {  // the next frame's first pass-halves
            pipe->resize(cs.size());
            for (size_t k = 0; k < cs.size(); ++k)
                BANDCHK(trace_front(cs[k], it0 + spp, 0, spp > 1, true, 1.0f / (float)spp, true, (*pipe)[k], spp == 1));
        }
        const int res = ((it0 + s) & 1) ? VXPT_BUF_RES_ODD : VXPT_BUF_RES_EVEN;
        if (s + 1 < spp) {
            // all but the last pass: the next pass's temporal taps' inputs -- the tap records on the
            // exchange stream once the pass's first half wrote them (beside its second half; the next
            // pass's k_restir waits for them), the reservoirs in stream order after its second half
            // (the next second half opens with k_restir: nothing to overlap them with; round 4 sent
            // both after the second half on the exchange stream)
            hipEvent_t recDone = cs.size() == 1 && cs[0]->comm ? cs[0]->frontDone[cs[0]->lastSet] : nullptr;
            BANDCHK(exchange_set(cs, {{VXPT_BUF_TAP_RECORD, traceRows}}, true, recDone));
            BANDCHK(exchange_set(cs, {{res, traceRows}}, false));
        } else {
            // the last pass: its planes for the denoiser, and the denoiser input (radiance, or the spp
            // average) for the firefly filter's 3x3 neighbours.  Its reservoirs go out at the trace
            // depth after the firefly filter has rewritten them (below); without the filter, here.
            for (vxpt_ctx *c : cs) c->denoiseInputIsAccum = spp > 1;
            std::vector<std::pair<int, int>> br{{VXPT_BUF_TAP_RECORD, traceRows}, {VXPT_BUF_ILLUM, 2},
                                                {res, p->enable_firefly_filter ? 2 : traceRows}};
            for (int b : kGbufPlanes) br.emplace_back(b, planeRows);
            BANDCHK(exchange_set(cs, br, false));
        }
    }
    for (size_t k = 0; k < cs.size(); ++k) {
        vxpt_ctx *c = cs[k];
        c->denoiseInputIsAccum = spp > 1;
        // the chain after the next frame's first pass-half (pipelined), so it runs alone -- with the
        // chain gate (without it the later first halves run beside the chain anyway: no wait)
        if (pipe && pipeNext && pipe->size() == cs.size() && chain_gate(c, spp))
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->frontDone[(*pipe)[k].set], 0));
        HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    }
    for (size_t k = 0; k < cs.size(); ++k)
        if (cs[k]->bst.on) BANDCHK(stat_mark(cs[k], cs[k]->stream, mk[3 * k + 1]));
    const int it = it0 + spp, used = it > 0 ? it - 1 : 0;
    std::vector<std::pair<int, int>> deferred;  // halo rows no pass reads before the next group
    auto exg = [&](std::vector<std::pair<int, int>> br) {
        br.insert(br.end(), deferred.begin(), deferred.end());
        deferred.clear();
        return exchange_set(cs, br);
    };
    auto to_rows = [](const std::vector<int> &bufs, int rows) {
        std::vector<std::pair<int, int>> br;
        for (int bf : bufs) br.emplace_back(bf, rows);
        return br;
    };
    if (!p->enable_firefly_filter) FOR_BANDS(run_pass(c, p, 11, 0, 0));
    if (p->enable_firefly_filter) {  // + world positions
        FOR_BANDS(run_pass(c, p, 0, used & 1, 0));
        // the filtered reservoirs (read by the next frame's first temporal taps) and radiance (read by
        // the history clamp's neighbourhood) ride along with the next group instead of one of their own
        deferred.emplace_back((used & 1) ? VXPT_BUF_RES_ODD : VXPT_BUF_RES_EVEN, traceRows);
        deferred.emplace_back(VXPT_BUF_ILLUM, 2);
    }
    const std::vector<int> hist(std::begin(kHistoryBufs), std::end(kHistoryBufs));
    if (frame == 0) {
        FOR_BANDS(run_pass(c, p, 12, 0, 0));
        BANDCHK(exg(to_rows(hist, histRows)));
    }
    // Ghost rows (the default chain, frames > 0): the history clamp and the a-trous steps compute the
    // rows the later steps read outside the band themselves (run_pass margins), so the chain exchanges
    // twice -- after the temporal pass and after the history fix -- instead of after every pass.  The
    // margins, backwards from the output (margin 0): a step at margin m reads its input at m + its reach
    // (a-trous rows of the step; 2 for the LDS a-trous and the clamp's 5x5), 8-aligned.  The history fix
    // (its taps 34 rows away) stays at margin 0: ghost rows for it would cost 34 more rows of every pass
    // before it.  Its inputs at the clamp's margin + 2 come in the two groups; the clamp's histories at
    // its margin serve the next frame's temporal pass (histRows <= that margin: no exchange).
    std::vector<int> atrousSteps;  // steps 2, 4, ..., 2^(2n+1): the last one (pass 10) writes the output
    for (int idx = 1; idx <= 2 * p->atrous_iteration_num + 1; ++idx) atrousSteps.push_back(1 << idx);
    std::vector<int> stepMargin(atrousSteps.size(), 0);
    int smemMargin = 0, clampMargin = 0;
    {
        int m = 0;
        for (int k = (int)atrousSteps.size() - 1; k >= 0; --k) {
            stepMargin[k] = m;
            m = (m + atrous_rows(atrousSteps[k]) + 7) / 8 * 8;
        }
        smemMargin = m;
        clampMargin = (smemMargin + 2 + 7) / 8 * 8;
    }
    const bool ghost = cs.size() > 0 && cs[0]->tune.ghost_rows && frame > 0 && p->enable_temporal_accumulation &&
                       p->enable_history_fix && p->enable_history_clamping && p->enable_spatial_filtering &&
                       p->atrous_iteration_num > 0 &&
                       // the clamp's pixel planes and the a-trous taps' world positions / normals, read at
                       // up to the LDS a-trous margin + 2, are there already (the last pass's planes, the
                       // firefly pass's positions)
                       clampMargin <= planeRows && smemMargin + 2 <= kWposHalo;
    int fin = 0;
    if (ghost) {
        FOR_BANDS(run_pass(c, p, 2, 0, 0));
        // the history fix's ping taps (34 rows) and the clamp's inputs at its margin: ping and the history
        // length at the pixel, the radiance in its 5x5 (the firefly-filtered values; the deferred 2-row
        // radiance entry is this one)
        std::vector<std::pair<int, int>> br{{VXPT_BUF_PING, std::max(34, clampMargin)}, {VXPT_BUF_PONG, 2},
                                            {VXPT_BUF_HIST_LEN, clampMargin}, {VXPT_BUF_ILLUM, clampMargin + 2}};
        for (const auto &d : deferred)
            if (d.first != VXPT_BUF_ILLUM) br.push_back(d);
        deferred.clear();
        BANDCHK(exchange_set(cs, br));
        FOR_BANDS(run_pass(c, p, 3, 0, 0));
        BANDCHK(exchange_set(cs, {{VXPT_BUF_PONG, clampMargin + 2}}));  // the clamp's 5x5 of the fixed history
        FOR_BANDS(run_pass(c, p, 4, 0, 0, clampMargin));
        if (histRows > clampMargin) BANDCHK(exchange_set(cs, to_rows(hist, histRows)));
        FOR_BANDS(run_pass(c, p, 5, 0, 0, smemMargin));
        for (size_t k = 0; k < atrousSteps.size(); ++k) {
            const int pass = k + 1 == atrousSteps.size() ? 10 : (k % 2 == 0 ? 6 : 7);
            FOR_BANDS(run_pass(c, p, pass, atrousSteps[k], it, stepMargin[k]));
        }
        for (vxpt_ctx *c : cs) c->haloHistRows = std::max(histRows, clampMargin);
        FOR_BANDS(run_pass(c, p, 14, 0, 0));
    }
    if (p->enable_temporal_accumulation && frame > 0 && !ghost) {
        FOR_BANDS(run_pass(c, p, 2, 0, 0));
        // HistoryFix taps: 2 x (2^3 + 1) rows of ping; pong for its 2-row stencils
        BANDCHK(exg({{VXPT_BUF_PING, 34}, {VXPT_BUF_PONG, 2}}));
        fin = 1;
        if (p->enable_history_fix) {
            FOR_BANDS(run_pass(c, p, 3, 0, 0));
            BANDCHK(exg({{VXPT_BUF_PONG, 2}}));
            fin = 2;
        }
        if (p->enable_history_clamping) {
            FOR_BANDS(run_pass(c, p, 4, 0, 0));
            BANDCHK(exg(to_rows(hist, histRows)));
            fin = 3;
        }
    }
    bool outDone = ghost;
    if (p->enable_spatial_filtering && !ghost) {
        FOR_BANDS(run_pass(c, p, 5, 0, 0));
        BANDCHK(exg({{VXPT_BUF_PING, atrous_rows(2)}}));
        fin = 1;
        if (p->atrous_iteration_num > 0) {
            int idx = 1, step = 2;
            while (idx < 2 * p->atrous_iteration_num) {
                FOR_BANDS(run_pass(c, p, 6, step, it));
                step = 1 << ++idx;
                BANDCHK(exg({{VXPT_BUF_PONG, atrous_rows(step)}}));
                FOR_BANDS(run_pass(c, p, 7, step, it));
                step = 1 << ++idx;
                BANDCHK(exg({{VXPT_BUF_PING, atrous_rows(step)}}));
            }
            FOR_BANDS(run_pass(c, p, 10, step, it));
            fin = 2;
            outDone = true;
        }
    }
    if (!deferred.empty()) BANDCHK(exg({}));  // nothing after the firefly pass exchanged (chain switches)
    if (!outDone) FOR_BANDS(run_pass(c, p, 13, fin, 0));
    if (!ghost) FOR_BANDS(run_pass(c, p, 14, 0, 0));
    for (vxpt_ctx *c : cs) {
        HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
        HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
    }
    for (size_t k = 0; k < cs.size(); ++k) {
        vxpt_ctx *c = cs[k];
        if (!c->bst.on) continue;
        BANDCHK(stat_mark(c, c->stream, mk[3 * k + 2]));
        c->bst.spans.push_back({mk[3 * k], mk[3 * k + 1], 2});
        c->bst.spans.push_back({mk[3 * k + 1], mk[3 * k + 2], 3});
        ++c->bst.frames;
    }
    if (!sync) return VXPT_OK;
    for (vxpt_ctx *c : cs) HIPCHK(c, hipStreamSynchronize(c->stream));
    band_timings(cs);
    for (vxpt_ctx *c : cs)
        if (c->bst.on) BANDCHK(stat_sync_fold(c));
    return VXPT_OK;
}

}  // namespace vx::host

// =====================================================================  C ABI
extern "C" {

int vxpt_set_band(vxpt_ctx *c, int row_begin, int row_end) {
    if (!c) return VXPT_ERR_ARG;
    if (row_end <= row_begin) { row_begin = 0; row_end = c->H; }
    // bands start on an 8-row boundary: 8x8 trace tiles and the firefly filter's 8x4 tiles stay whole
    if (row_begin < 0 || row_end > c->H || (row_begin & 7) || ((row_end & 7) && row_end != c->H))
        return fail(c, VXPT_ERR_ARG, "band rows must be 8-aligned and inside the frame");
    c->rowBegin = row_begin;
    c->rowEnd = row_end;
    return VXPT_OK;
}

int vxpt_row_bytes(vxpt_ctx *c, int which) {
    void *p, *mirror;
    size_t n;
    if (!c || !buffer_ptr(c, which, p, n, false, &mirror) || (which >= 32 && which <= 34) ||
        which == VXPT_BUF_RESERVOIRS)
        return VXPT_ERR_ARG;
    return (int)(n / (size_t)c->H);
}

int vxpt_copy_rows(vxpt_ctx *c, int which, int y, int rows, void *dev, int to_buffer) {
    if (!c || !dev || rows < 0 || y < 0 || y + rows > c->H) return VXPT_ERR_ARG;
    const int rb = vxpt_row_bytes(c, which);
    if (rb <= 0) return fail(c, VXPT_ERR_ARG, "buffer has no row layout");
    void *p, *mirror;
    size_t n;
    buffer_ptr(c, which, p, n, false, &mirror);
    HIPCHK(c, hipSetDevice(c->dev));
    char *row = static_cast<char *>(p) + (size_t)y * rb;
    if (to_buffer) gbuf_written(c, which);
    if (to_buffer) HIPCHK(c, hipMemcpyAsync(row, dev, (size_t)rows * rb, hipMemcpyDeviceToDevice, c->stream));
    else HIPCHK(c, hipMemcpyAsync(dev, row, (size_t)rows * rb, hipMemcpyDeviceToDevice, c->stream));
    return VXPT_OK;
}

// the halo exchange of the band schedule for the buffers of `mask` (bit b = buffer id b < 32), over the
// context's RCCL communicator, enqueued on its stream
int vxpt_exchange_halo(vxpt_ctx *c, uint32_t mask, int rows) {
    if (!c || rows < 0) return VXPT_ERR_ARG;
    if (c->nranks <= 1 || mask == 0 || rows == 0) return VXPT_OK;
    if (!c->comm) return fail(c, VXPT_ERR_STATE, "no band communicator (vxpt_band_comm_init; linked contexts exchange inside vxpt_render_frame_linked)");
    std::vector<std::pair<int, int>> br;
    for (int b = 0; b < 32; ++b) {
        if (!((mask >> b) & 1u)) continue;
        void *ptr, *mirror;
        size_t n;
        if (!buffer_ptr(c, b, ptr, n, false, &mirror) || b == VXPT_BUF_RESERVOIRS)
            return fail(c, VXPT_ERR_ARG, "buffer has no row layout");
        gbuf_written(c, b);
        br.emplace_back(b, rows);
    }
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<vxpt_ctx *> cs{c};
    return exchange_set(cs, br, false);
}

// A banded frame's post-process (PostProcessingPipeline::Execute over bands): the denoiser
// output's 1-row halo (the bloom extract's vertical neighbours), each band's histogram + bloom
// rows, the histogram (+ sun flag) summed over the bands -- an RCCL all-reduce of 257 u32, or a
// host sum for linked contexts -- so that every band adapts the same exposure, the horizontally
// blurred bloom's halo for the vertical taps, then exposure + compose of the band's rows.
int band_post(std::vector<vxpt_ctx *> &cs, const vxpt_post_params *pp, float dtMs) {
    std::vector<PostArgs> as(cs.size());
    for (size_t k = 0; k < cs.size(); ++k) BANDCHK(post_args(cs[k], pp, dtMs, as[k]));
    const int half = post_bloom_half(as[0]);
    if (half > 0 && half > cs[0]->rowEnd - cs[0]->rowBegin)
        return fail(cs[0], VXPT_ERR_ARG, "bloom radius exceeds the band height");
    BANDCHK(exchange_set(cs, {{VXPT_BUF_OUTPUT, 1}}));
    for (size_t k = 0; k < cs.size(); ++k) HIPCHK(cs[k], launch_post_phase1(as[k], cs[k]->stream));
    const bool reduce = as[0].p.enableAutoExposure || (as[0].p.enableLensFlare && as[0].sunOnScreen);
    if (reduce) {
        if (cs.size() == 1 && cs[0]->comm) {
            vxpt_ctx *c = cs[0];
            if (ncclAllReduce(c->postHist, c->postHist, kPostHist, ncclUint32, ncclSum, c->comm, c->stream) != ncclSuccess)
                return fail(c, VXPT_ERR_HIP, "ncclAllReduce (post histogram)");
        } else {
            std::vector<unsigned> sum(kPostHist, 0u), h(kPostHist);
            for (vxpt_ctx *c : cs) {
                HIPCHK(c, hipMemcpyAsync(h.data(), c->postHist, kPostHist * 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                for (int i = 0; i < kPostHist; ++i) sum[i] += h[i];
            }
            for (vxpt_ctx *c : cs) {
                HIPCHK(c, hipMemcpyAsync(c->postHist, sum.data(), kPostHist * 4, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
        }
    }
    if (half > 0) BANDCHK(exchange_set(cs, {{VXPT_BUF_BLOOM, half}}));
    for (size_t k = 0; k < cs.size(); ++k) HIPCHK(cs[k], launch_post_phase2(as[k], cs[k]->stream));
    return VXPT_OK;
}

int vxpt_postprocess_linked(vxpt_ctx **cs, int n, const vxpt_post_params *pp, float dtMs) {
    if (!cs || n < 1) return VXPT_ERR_ARG;
    std::vector<vxpt_ctx *> v(cs, cs + n);
    for (int k = 0; k < n; ++k)
        if (!cs[k] || cs[k]->rank != k || cs[k]->nranks != n) return VXPT_ERR_STATE;
    HIPCHK(cs[0], hipSetDevice(cs[0]->dev));
    if (int r = band_post(v, pp, dtMs)) return r;
    for (vxpt_ctx *c : v) HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}


int vxpt_band_comm_id(void *id, size_t bytes) {
    if (!id || bytes < sizeof(ncclUniqueId)) return VXPT_ERR_ARG;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return VXPT_ERR_HIP;
    std::memcpy(id, &u, sizeof(u));
    return VXPT_OK;
}

int vxpt_band_comm_init(vxpt_ctx *c, const void *id, size_t bytes, int nranks, int rank) {
    return vxpt_band_comm_init_rows(c, id, bytes, nranks, rank, nullptr);
}

int vxpt_band_comm_init_rows(vxpt_ctx *c, const void *id, size_t bytes, int nranks, int rank, const int32_t *row_splits) {
    if (!c || !id || bytes < sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<int> s = equal_splits(c->H, nranks);
    if (row_splits) {
        if (!splits_valid(row_splits, nranks, c->H, kTraceHalo))
            return fail(c, VXPT_ERR_ARG, "row_splits: 0 = s[0] < ... < s[n] = height, 8-aligned, bands >= 72 rows");
        s.assign(row_splits, row_splits + nranks + 1);
    }
    const int y0 = s[rank], y1 = s[rank + 1];
    if (nranks > 1 && (y1 - y0 < kTraceHalo))
        return fail(c, VXPT_ERR_ARG, "bands must be at least 72 rows tall (ReSTIR halo)");
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    if (c->comm) ncclCommDestroy(c->comm);
    c->comm = nullptr;
    c->exDoneRec = false;
    if (ncclCommInitRank(&c->comm, nranks, u, rank) != ncclSuccess) return fail(c, VXPT_ERR_HIP, "ncclCommInitRank");
    if (!c->commStream) HIPCHK(c, hipStreamCreateWithFlags(&c->commStream, hipStreamNonBlocking));
    // the exchange stream's events keep the system-scope fence: the rows a peer GPU wrote over xGMI must
    // be visible to the kernel that waits for them (without it one band measured ~1 % faster, within the
    // run-to-run spread: not worth a stale-cache risk)
    if (!c->haloReady) HIPCHK(c, hipEventCreateWithFlags(&c->haloReady, hipEventDisableTiming));
    if (!c->haloDone) HIPCHK(c, hipEventCreateWithFlags(&c->haloDone, hipEventDisableTiming));
    if (!c->exDone) HIPCHK(c, hipEventCreateWithFlags(&c->exDone, hipEventDisableTiming | hipEventDisableSystemFence));
    c->nranks = nranks;
    c->rank = rank;
    c->splits = s;
    return vxpt_set_band(c, y0, y1);
}

int vxpt_band_link(vxpt_ctx **cs, int n) { return vxpt_band_link_rows(cs, n, nullptr); }

int vxpt_band_stats_enable(vxpt_ctx *c, int on) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // no recorded event of the last collection pending
    if (c->commStream) HIPCHK(c, hipStreamSynchronize(c->commStream));
    auto &b = c->bst;
    b.on = on != 0;
    b.used = 0;
    b.spans.clear();
    for (double &m : b.ms) m = 0.0;
    b.frames = b.groups = b.groupsOrdered = 0;
    b.up = b.down = 0.0;
    return VXPT_OK;
}

int vxpt_band_stats(vxpt_ctx *c, vxpt_band_stat *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    if (int r = stat_sync_fold(c)) return r;
    const auto &b = c->bst;
    vxpt_band_stat s{};
    s.frames = b.frames;
    s.groups = b.groups;
    s.groups_ordered = b.groupsOrdered;
    s.bytes_up = b.up;
    s.bytes_down = b.down;
    s.row_begin = c->rowBegin;
    s.row_end = c->rowEnd;
    s.exchange_ms = (float)b.ms[0];
    s.exchange_overlap_ms = (float)b.ms[1];
    s.trace_ms = (float)b.ms[2];
    s.denoise_ms = (float)b.ms[3];
    *out = s;
    return VXPT_OK;
}

int vxpt_band_link_rows(vxpt_ctx **cs, int n, const int32_t *row_splits) {
    if (!cs || n < 1 || !cs[0]) return VXPT_ERR_ARG;
    std::vector<int> s = equal_splits(cs[0]->H, n);
    if (row_splits) {
        if (!splits_valid(row_splits, n, cs[0]->H, kTraceHalo))
            return fail(cs[0], VXPT_ERR_ARG, "row_splits: 0 = s[0] < ... < s[n] = height, 8-aligned, bands >= 72 rows");
        s.assign(row_splits, row_splits + n + 1);
    }
    for (int k = 0; k < n; ++k) {
        vxpt_ctx *c = cs[k];
        if (!c || c->W != cs[0]->W || c->H != cs[0]->H) return VXPT_ERR_ARG;
        const int y0 = s[k], y1 = s[k + 1];
        if (n > 1 && (y1 - y0 < kTraceHalo)) return fail(c, VXPT_ERR_ARG, "bands must be at least 72 rows tall");
        c->nranks = n;
        c->rank = k;
        c->splits = s;
        c->linked.assign(cs, cs + n);
        if (int r = vxpt_set_band(c, y0, y1)) return r;
    }
    return VXPT_OK;
}

// Every band's rows of a buffer into the root's buffer (the frame's output for one writer).  RCCL:
// grouped ncclSend to the root / ncclRecv of each band at the root, on the context streams.

int band_gather(std::vector<vxpt_ctx *> &cs, int which, int root) {
    vxpt_ctx *c0 = cs[0];
    const int world = c0->nranks;
    if (root < 0 || root >= world) return fail(c0, VXPT_ERR_ARG, "root rank out of range");
    {
        void *ptr, *mirror;
        size_t n;
        if (!buffer_ptr(c0, which, ptr, n, false, &mirror) || which == VXPT_BUF_RESERVOIRS || (which >= 32 && which <= 34))
            return fail(c0, VXPT_ERR_ARG, "buffer has no row layout (or is not allocated yet)");
    }
    if (cs.size() == 1 && c0->comm) {
        size_t rb;
        // behind every halo group on the exchange stream too: one communicator's groups run in issue
        // order on every rank (a gather beside a pending halo group could pair differently per rank)
        if (c0->haloPending) HIPCHK(c0, hipStreamWaitEvent(c0->stream, c0->haloDone, 0));
        if (ncclGroupStart() != ncclSuccess) return fail(c0, VXPT_ERR_HIP, "ncclGroupStart");
        ncclResult_t rc = ncclSuccess;
        if (c0->rank == root) {
            const std::vector<int> sp = splits_of(c0);
            for (int r = 0; r < world && rc == ncclSuccess; ++r) {
                const int y0 = sp[r], y1 = sp[r + 1];
                if (r == root || y1 <= y0) continue;
                char *dst = buffer_rows(c0, which, y0, rb);
                rc = ncclRecv(dst, (size_t)(y1 - y0) * rb, ncclUint8, r, c0->comm, c0->stream);
            }
        } else if (c0->rowEnd > c0->rowBegin) {
            char *src = buffer_rows(c0, which, c0->rowBegin, rb);
            rc = ncclSend(src, (size_t)(c0->rowEnd - c0->rowBegin) * rb, ncclUint8, root, c0->comm, c0->stream);
        }
        const ncclResult_t re = ncclGroupEnd();
        if (rc != ncclSuccess)
            return fail(c0, VXPT_ERR_HIP, std::string("ncclSend/ncclRecv (gather): ") + ncclGetErrorString(rc));
        if (re != ncclSuccess)
            return fail(c0, VXPT_ERR_HIP, std::string("ncclGroupEnd (gather): ") + ncclGetErrorString(re));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));
        return VXPT_OK;
    }
    for (vxpt_ctx *c : cs) HIPCHK(c, hipStreamSynchronize(c->stream));
    vxpt_ctx *dst = cs[root];
    for (int r = 0; r < (int)cs.size(); ++r) {
        if (r == root || cs[r]->rowEnd <= cs[r]->rowBegin) continue;
        size_t rb;
        char *d = buffer_rows(dst, which, cs[r]->rowBegin, rb);
        const char *src = buffer_rows(cs[r], which, cs[r]->rowBegin, rb);
        HIPCHK(dst, hipMemcpyAsync(d, src, (size_t)(cs[r]->rowEnd - cs[r]->rowBegin) * rb, hipMemcpyDeviceToDevice,
                                   dst->stream));
    }
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    return VXPT_OK;
}

int vxpt_band_gather(vxpt_ctx *c, int which, int root) {
    if (!c) return VXPT_ERR_ARG;
    if (c->nranks <= 1) return VXPT_OK;
    if (!c->comm) return fail(c, VXPT_ERR_STATE, "no band communicator (linked contexts: vxpt_band_gather_linked)");
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<vxpt_ctx *> cs{c};
    return band_gather(cs, which, root);
}

int vxpt_band_gather_linked(vxpt_ctx **cs, int n, int which, int root) {
    if (!cs || n < 1) return VXPT_ERR_ARG;
    for (int k = 0; k < n; ++k)
        if (!cs[k] || cs[k]->rank != k || cs[k]->nranks != n) return VXPT_ERR_STATE;
    if (n == 1) return VXPT_OK;
    HIPCHK(cs[0], hipSetDevice(cs[0]->dev));
    std::vector<vxpt_ctx *> v(cs, cs + n);
    return band_gather(v, which, root);
}

int vxpt_band_rows(int height, int nranks, int rank, int *row_begin, int *row_end) {
    if (height < 1 || nranks < 1 || rank < 0 || rank >= nranks || !row_begin || !row_end) return VXPT_ERR_ARG;
    band_rows(height, nranks, rank, *row_begin, *row_end);
    return VXPT_OK;
}

// Cost-balanced band boundaries from measured band times.  block_cost holds the frame's cost per
// 8-row block (ceil(height / 8) entries, carried between calls; a negative first entry = no estimate
// yet): each band's blocks are scaled so they sum to its measured time (a band without an estimate
// spreads its time evenly), then the boundaries go where the cumulative cost crosses k / n of the
// total, on block boundaries, every band keeping >= 72 rows.
int vxpt_band_balance(int height, int nranks, const int32_t *row_splits, const float *band_ms, float *block_cost,
                      int32_t *out_splits) {
    if (height < 1 || nranks < 1 || !row_splits || !band_ms || !block_cost || !out_splits) return VXPT_ERR_ARG;
    if (!splits_valid(row_splits, nranks, height, nranks > 1 ? kTraceHalo : 1)) return VXPT_ERR_ARG;
    const int nb = (height + 7) / 8;
    if (nranks > 1 && (int64_t)nranks * kTraceHalo > height) return VXPT_ERR_ARG;
    if (block_cost[0] < 0.0f)
        for (int b = 0; b < nb; ++b) block_cost[b] = 0.0f;
    for (int k = 0; k < nranks; ++k) {
        if (!(band_ms[k] >= 0.0f)) return VXPT_ERR_ARG;
        const int b0 = row_splits[k] / 8, b1 = (row_splits[k + 1] + 7) / 8;
        double cur = 0.0;
        for (int b = b0; b < b1; ++b) cur += block_cost[b];
        for (int b = b0; b < b1; ++b)
            block_cost[b] = cur > 0.0 ? (float)(block_cost[b] * (band_ms[k] / cur)) : band_ms[k] / (float)(b1 - b0);
    }
    std::vector<double> cum(nb + 1, 0.0);
    for (int b = 0; b < nb; ++b) cum[b + 1] = cum[b] + block_cost[b];
    const int minBlocks = nranks > 1 ? kTraceHalo / 8 : 1;
    out_splits[0] = 0;
    int prev = 0;
    for (int k = 1; k < nranks; ++k) {
        const double target = cum[nb] * k / nranks;
        const int lo = prev + minBlocks;
        const int hi = (height - (nranks - k) * kTraceHalo) / 8;  // the bands after it keep 72 rows
        int best = lo;
        for (int b = lo; b <= hi; ++b)
            if (std::fabs(cum[b] - target) < std::fabs(cum[best] - target)) best = b;
        out_splits[k] = best * 8;
        prev = best;
    }
    out_splits[nranks] = height;
    return VXPT_OK;
}

int vxpt_halo_plan(int height, int nranks, int rank, int rows, int32_t *out, int *n_entries) {
    if (height < 1 || nranks < 1 || rank < 0 || rank >= nranks || rows < 0 || !out || !n_entries) return VXPT_ERR_ARG;
    const std::vector<Halo> plan = halo_plan(equal_splits(height, nranks), rank, rows);
    for (size_t k = 0; k < plan.size(); ++k) {
        const Halo &h = plan[k];
        const int32_t e[5] = {h.peer, h.sy, h.sn, h.ry, h.rn};
        std::memcpy(out + 5 * k, e, sizeof(e));
    }
    *n_entries = (int)plan.size();
    return VXPT_OK;
}

int vxpt_band_halo_rows(const vxpt_camera *cur, const vxpt_camera *prev, int width, int height, int nranks,
                        int *trace_rows, int *history_rows) {
    if (!cur || width < 1 || height < 1 || nranks < 1 || !trace_rows || !history_rows) return VXPT_ERR_ARG;
    const CamDev c = make_camera(width, height, *cur, nullptr, nullptr);
    const CamDev pc = make_camera(width, height, prev ? *prev : *cur, nullptr, nullptr);
    std::string err;
    return band_halo_rows(c, pc, width, height, equal_splits(height, nranks), *trace_rows, *history_rows, err)
               ? VXPT_OK : VXPT_ERR_STATE;
}

int vxpt_band_halo_rows_near(const vxpt_camera *cur, const vxpt_camera *prev, int width, int height, int nranks,
                             float near_depth, int *trace_rows, int *history_rows) {
    if (!cur || width < 1 || height < 1 || nranks < 1 || !trace_rows || !history_rows) return VXPT_ERR_ARG;
    const CamDev c = make_camera(width, height, *cur, nullptr, nullptr);
    const CamDev pc = make_camera(width, height, prev ? *prev : *cur, nullptr, nullptr);
    std::string err;
    return band_halo_rows(c, pc, width, height, equal_splits(height, nranks), *trace_rows, *history_rows, err,
                          near_depth) ? VXPT_OK : VXPT_ERR_STATE;
}

int vxpt_render_frame_linked(vxpt_ctx **cs, int n, const vxpt_denoise_params *p, int32_t frameNum, int32_t spp) {
    if (!cs || n < 1 || spp < 1) return VXPT_ERR_ARG;
    std::vector<vxpt_ctx *> v(cs, cs + n);
    for (int k = 0; k < n; ++k)
        if (!cs[k] || cs[k]->rank != k || cs[k]->nranks != n) return VXPT_ERR_STATE;
    HIPCHK(cs[0], hipSetDevice(cs[0]->dev));
    return band_frame(v, denoise_or_yaml(v[0], p), frameNum, spp);
}

// the banded vxpt_render_frames' pipelined schedule (band_frame's pipe) over linked contexts
int vxpt_render_frames_linked(vxpt_ctx **cs, int n, const vxpt_denoise_params *p, int32_t frame0, int32_t nFrames,
                              int32_t spp) {
    if (!cs || n < 1 || spp < 1 || nFrames < 1 || frame0 < 0) return VXPT_ERR_ARG;
    std::vector<vxpt_ctx *> v(cs, cs + n);
    for (int k = 0; k < n; ++k)
        if (!cs[k] || cs[k]->rank != k || cs[k]->nranks != n) return VXPT_ERR_STATE;
    HIPCHK(cs[0], hipSetDevice(cs[0]->dev));
    std::vector<PassPlan> pipe;  // every band's next-frame first pass-halves
    for (int f = 0; f < nFrames; ++f)
        if (int r = band_frame(v, denoise_or_yaml(v[0], p), frame0 + f, spp, false, &pipe, f + 1 < nFrames)) return r;
    for (vxpt_ctx *c : v) HIPCHK(c, hipStreamSynchronize(c->stream));
    band_timings(v);
    for (vxpt_ctx *c : v)
        if (c->bst.on) BANDCHK(stat_sync_fold(c));
    return VXPT_OK;
}

}  // extern "C"
