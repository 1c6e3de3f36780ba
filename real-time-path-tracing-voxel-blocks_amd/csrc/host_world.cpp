// vxpt -- host runtime, the voxel world: the DDA tables and host mirrors built on the host or on the device
// (world.hip), single and batched block edits, picking, the nearest-surface bound, chunk files.
#include <algorithm>
#include <array>
#include <cctype>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "host_ctx.hpp"
#include "world_build.hpp"

namespace {

// brick coordinates (4^3 cells) -> cellMask / octant-table index (16^3 macro cell m, brick lb)
inline size_t brick_lin(const vxpt_ctx *c, int bx, int by, int bz) {
    const size_t m = (size_t)(bx >> 2) + (size_t)(c->cx * 2) * ((bz >> 2) + (size_t)(c->cz * 2) * (by >> 2));
    return m * 64 + (size_t)((bx & 3) + 4 * ((bz & 3) + 4 * (by & 3)));
}
inline bool is_cube(int id) { return id >= 1 && id <= 12; }

// Per-octant empty-box sizes: for every 4^3 brick and each of the 8 ray octants,
// S = the edge (in bricks) of the largest brick-aligned cube with that brick at its
// corner, extending in the octant's directions, that holds no cube cell (0 = the
// brick is occupied; out-of-world counts as empty; capped at 255).  A ray in that
// octant can leave the whole cube in one jump.  3-D "largest empty square"
// recurrence S = 1 + min(S of the 7 forward neighbours), evaluated over the brick box
// [x0,x1] x [y0,y1] x [z0,z1] against the octant's direction; bricks outside the box
// keep their values (an edit recomputes only the bricks behind it).
void octant_fill(vxpt_ctx *c, int oct, int x0, int x1, int y0, int y1, int z0, int z1) {
    const int BX = c->cx * 8, BY = c->cy * 8, BZ = c->cz * 8;
    const size_t nB = (size_t)BX * BY * BZ;
    uint8_t *S = c->hOd.data() + (size_t)oct * nB;
    const int sx = (oct & 1) ? 1 : -1, sy = (oct & 2) ? 1 : -1, sz = (oct & 4) ? 1 : -1;
    auto get = [&](int x, int y, int z) -> int {
        if (x < 0 || y < 0 || z < 0 || x >= BX || y >= BY || z >= BZ) return 255;
        return S[brick_lin(c, x, y, z)];
    };
    for (int iy = 0; iy <= y1 - y0; ++iy)
        for (int iz = 0; iz <= z1 - z0; ++iz)
            for (int ix = 0; ix <= x1 - x0; ++ix) {
                const int x = sx > 0 ? x1 - ix : x0 + ix, y = sy > 0 ? y1 - iy : y0 + iy, z = sz > 0 ? z1 - iz : z0 + iz;
                const size_t b = brick_lin(c, x, y, z);
                int v = 0;
                if (!c->hCell[b]) {
                    int mn = 255;
                    for (int k = 1; k < 8; ++k)
                        mn = std::min(mn, get(x + ((k & 1) ? sx : 0), y + ((k & 2) ? sy : 0), z + ((k & 4) ? sz : 0)));
                    v = std::min(255, 1 + mn);
                }
                S[b] = (uint8_t)v;
            }
}

}  // namespace

namespace vx::host {

// the box tables over brick box [x0,x1] x [y0,y1] x [z0,z1] of octant oct, from the cube tables and
// the occupancy prefix counts (both current)
void box_fill(vxpt_ctx *c, int oct, int x0, int x1, int y0, int y1, int z0, int z1) {
    const int boxCap = c->boxCap, boxCapUp = c->boxCapUp;
    const size_t nB = (size_t)c->cx * 8 * c->cy * 8 * c->cz * 8;
    for (int y = y0; y <= y1; ++y)
        for (int z = z0; z <= z1; ++z)
            for (int x = x0; x <= x1; ++x) {
                const size_t b = brick_lin(c, x, y, z);
                c->hBox[oct * nB + b] = grow_box(c->brickPrefix, x, y, z, oct, c->hOd[oct * nB + b], boxCap, boxCapUp);
            }
}
void brick_prefix(vxpt_ctx *c) {
    c->brickPrefix.build(c->cx * 8, c->cy * 8, c->cz * 8,
                         [&](int x, int y, int z) { return c->hCell[brick_lin(c, x, y, z)] != 0; });
}

}  // namespace vx::host

namespace {

inline int top_block(const vxpt_ctx *c, int x, int y, int z) {
    const int tx = (c->cx * 32 + 63) / 64, tz = (c->cz * 32 + 63) / 64;
    return (x >> 6) + tx * ((z >> 6) + tz * (y >> 6));
}
void refresh_top(vxpt_ctx *c) {
    c->top = 0;
    for (size_t t = 0; t < c->topCount.size() && t < 64; ++t)
        if (c->topCount[t]) c->top |= 1ull << t;
}

// DDA acceleration layout (WorldDev) from chunk-major ids, built in the host mirrors and uploaded
// the sky exit's table: for each x / z direction quadrant q ((dx > 0) | (dz > 0) << 1) and brick column,
// the highest 1 + cube row over the columns a walk in that quadrant can still reach (x, z not moving
// against the ray: a suffix maximum along each axis), uploaded on the context stream
int upload_sky_top(vxpt_ctx *c) {
    const int nbx = c->cx * 8, nbz = c->cz * 8;
    c->hSkyTop.assign((size_t)4 * nbx * nbz, 0);
    for (int q = 0; q < 4; ++q) {
        const bool px = q & 1, pz = q & 2;
        uint16_t *t = c->hSkyTop.data() + (size_t)q * nbx * nbz;
        for (int kz = 0; kz < nbz; ++kz)
            for (int kx = 0; kx < nbx; ++kx) {
                // walk the columns from the far corner of the quadrant towards its origin
                const int bz = pz ? nbz - 1 - kz : kz, bx = px ? nbx - 1 - kx : kx;
                const int fz = pz ? bz + 1 : bz - 1, fx = px ? bx + 1 : bx - 1;  // the next column along z / x
                uint16_t m = c->colTop[(size_t)bz * nbx + bx];
                if (fz >= 0 && fz < nbz) m = std::max(m, t[(size_t)fz * nbx + bx]);
                if (fx >= 0 && fx < nbx) m = std::max(m, t[(size_t)bz * nbx + fx]);
                t[(size_t)bz * nbx + bx] = m;
            }
    }
    return upload_vec(c, c->skyTop, c->hSkyTop.data(), c->hSkyTop.size());
}

// the host mirrors of a world (both build modes keep them: picking, vxpt_nearest_surface, chunk files
// and the instance refresh read them, and an edit updates them in O(1))
void build_mirrors(vxpt_ctx *c, const uint8_t *ids) {
    const int wx = c->cx * 32, wy = c->cy * 32, wz = c->cz * 32;
    const int mx = wx / 16, my = wy / 16, mz = wz / 16;
    c->hMacro.assign((size_t)mx * my * mz, 0ull);
    c->hBricks.assign((size_t)wx * wy * wz, 0);
    c->hCell.assign((size_t)mx * my * mz * 64, 0ull);
    const int tx = (wx + 63) / 64, ty = (wy + 63) / 64, tz = (wz + 63) / 64;
    c->topCount.assign((size_t)tx * ty * tz, 0);
    c->hNonAir.assign((size_t)mx * my * mz * 64, 0);
    c->colTop.assign((size_t)(wx >> 2) * (wz >> 2), 0);
    for (int y = 0; y < wy; ++y)
        for (int z = 0; z < wz; ++z)
            for (int x = 0; x < wx; ++x) {
                const int ch = (x >> 5) + c->cx * ((z >> 5) + c->cz * (y >> 5));
                const uint8_t id = ids[(size_t)ch * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))];
                if (!id) continue;
                const size_t b = brick_lin(c, x >> 2, y >> 2, z >> 2);
                const int lc = (x & 3) + 4 * ((z & 3) + 4 * (y & 3));
                c->hBricks[b * 64 + lc] = id;
                c->hNonAir[b]++;
                // only cube ids (1..12) make a brick visible to the DDA; other ids are empty for it
                if (is_cube(id)) {
                    c->hMacro[b / 64] |= 1ull << (b % 64);
                    c->hCell[b] |= 1ull << lc;
                    c->topCount[top_block(c, x, y, z)]++;
                    uint16_t &ct = c->colTop[(size_t)(z >> 2) * (wx >> 2) + (x >> 2)];
                    ct = std::max<uint16_t>(ct, (uint16_t)(y + 1));
                }
            }
    c->topValid = (tx * ty * tz <= 64) ? 1 : 0;
    refresh_top(c);
}

int build_occupancy(vxpt_ctx *c, const uint8_t *ids) {
    const int wx = c->cx * 32, wy = c->cy * 32, wz = c->cz * 32;
    build_mirrors(c, ids);
    if (int r = upload_sky_top(c)) return r;
    const int BX = wx / 4, BY = wy / 4, BZ = wz / 4;
    const size_t nB = (size_t)BX * BY * BZ;
    c->hOd.assign(8 * nB, 0);
    for (int oct = 0; oct < 8; ++oct) octant_fill(c, oct, 0, BX - 1, 0, BY - 1, 0, BZ - 1);
    c->nBricks = (int)nB;
    if (int r = upload_vec(c, c->bdist, c->hOd.data(), c->hOd.size())) return r;
    if (c->useBoxes) {
        brick_prefix(c);
        c->hBox.assign(8 * nB, 0u);
        for (int oct = 0; oct < 8; ++oct) box_fill(c, oct, 0, BX - 1, 0, BY - 1, 0, BZ - 1);
        if (int r = upload_vec(c, c->bbox, c->hBox.data(), c->hBox.size())) return r;
    }
    if (int r = upload_vec(c, c->bricks, c->hBricks.data(), c->hBricks.size())) return r;
    if (int r = upload_vec(c, c->macro, c->hMacro.data(), c->hMacro.size())) return r;
    if (int r = upload_vec(c, c->cellMask, c->hCell.data(), c->hCell.size())) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// One voxel edit (VoxelEngine::setVoxelAtGlobal, VoxelEngine.cu:265-276, and the uninstanced
// face-mesh update updateSingleVoxelGlobal, VoxelSceneGen.cu:643-786, whose DDA equivalent is
// this): the id in both layouts, the brick's cube mask, and -- when the brick turns occupied or
// empty -- its macro bit, the 64^3 block bit and the octant tables of the bricks behind it.
int set_block(vxpt_ctx *c, int x, int y, int z, int id) {
    const int wx = c->cx * 32, wy = c->cy * 32, wz = c->cz * 32;
    if (x < 0 || y < 0 || z < 0 || x >= wx || y >= wy || z >= wz || id < 0 || id > 255)
        return fail(c, VXPT_ERR_ARG, "block position or id out of range");
    const size_t ci = (size_t)((x >> 5) + c->cx * ((z >> 5) + c->cz * (y >> 5))) * 32768 + (x & 31) +
                      32 * ((z & 31) + 32 * (y & 31));
    const int old = c->hIds[ci];
    if (old == id) return 0;
    hipStream_t st = c->stream;
    c->hIds[ci] = (uint8_t)id;
    ++c->worldVersion;
    HIPCHK(c, hipMemcpyAsync(c->voxels.p + ci, &c->hIds[ci], 1, hipMemcpyHostToDevice, st));
    const size_t b = brick_lin(c, x >> 2, y >> 2, z >> 2);
    const int lc = (x & 3) + 4 * ((z & 3) + 4 * (y & 3));
    c->hBricks[b * 64 + lc] = (uint8_t)id;
    c->hNonAir[b] += (id != 0 ? 1 : 0) - (old != 0 ? 1 : 0);
    HIPCHK(c, hipMemcpyAsync(c->bricks.p + b * 64 + lc, &c->hBricks[b * 64 + lc], 1, hipMemcpyHostToDevice, st));
    if (is_cube(old) != is_cube(id)) {
        const uint64_t before = c->hCell[b];
        c->hCell[b] = is_cube(id) ? (before | (1ull << lc)) : (before & ~(1ull << lc));
        HIPCHK(c, hipMemcpyAsync(c->cellMask.p + b, &c->hCell[b], 8, hipMemcpyHostToDevice, st));
        c->topCount[top_block(c, x, y, z)] += is_cube(id) ? 1 : -1;
        refresh_top(c);
        if (is_cube(id) && c->colTop[(size_t)(z >> 2) * (wx >> 2) + (x >> 2)] < y + 1) {
            c->colTop[(size_t)(z >> 2) * (wx >> 2) + (x >> 2)] = (uint16_t)(y + 1);
            if (int r = upload_sky_top(c)) return r;
        }
        if ((before != 0) != (c->hCell[b] != 0)) {
            const size_t m = b / 64;
            c->hMacro[m] = c->hCell[b] ? (c->hMacro[m] | (1ull << (b % 64))) : (c->hMacro[m] & ~(1ull << (b % 64)));
            HIPCHK(c, hipMemcpyAsync(c->macro.p + m, &c->hMacro[m], 8, hipMemcpyHostToDevice, st));
            const int bx = x >> 2, by = y >> 2, bz = z >> 2, BX = c->cx * 8, BY = c->cy * 8, BZ = c->cz * 8;
            for (int oct = 0; oct < 8; ++oct)
                octant_fill(c, oct, (oct & 1) ? 0 : bx, (oct & 1) ? bx : BX - 1, (oct & 2) ? 0 : by,
                            (oct & 2) ? by : BY - 1, (oct & 4) ? 0 : bz, (oct & 4) ? bz : BZ - 1);
            HIPCHK(c, hipMemcpyAsync(c->bdist.p, c->hOd.data(), c->hOd.size(), hipMemcpyHostToDevice, st));
            if (c->useBoxes) {  // the boxes that could reach the brick: the same bricks behind it
                brick_prefix(c);
                for (int oct = 0; oct < 8; ++oct)
                    box_fill(c, oct, (oct & 1) ? 0 : bx, (oct & 1) ? bx : BX - 1, (oct & 2) ? 0 : by,
                             (oct & 2) ? by : BY - 1, (oct & 4) ? 0 : bz, (oct & 4) ? bz : BZ - 1);
                HIPCHK(c, hipMemcpyAsync(c->bbox.p, c->hBox.data(), c->hBox.size() * 4, hipMemcpyHostToDevice, st));
            }
        }
    }
    // the mirrors are the copies' sources: let them land before the host edits them again
    HIPCHK(c, hipStreamSynchronize(st));
    // OptixRenderer::update (:916-919): after a geometry change the previous frame's scene is
    // gone, so the next pass's ReSTIR temporal visibility rays (closesthit.cu:736-755) miss
    c->prevSceneEmpty = 1;
    return 0;
}

// ---------------------------------------------------------------- tables on the device (world.hip)
WbWorld wb_world(const vxpt_ctx *c) {
    WbWorld w{};
    w.ids = c->voxels.p;
    w.bricks = c->bricks.p;
    w.macro = c->macro.p;
    w.cellMask = c->cellMask.p;
    w.bdist = c->bdist.p;
    w.bbox = c->useBoxes ? c->bbox.p : nullptr;
    w.skyTop = c->skyTop.p;
    w.colTop = c->dColTop.p;
    w.prefix = c->dPrefix.p;
    w.cx = c->cx; w.cy = c->cy; w.cz = c->cz;
    w.cap = c->boxCap; w.capUp = c->boxCapUp;
    return w;
}
WbRanges wb_whole(const vxpt_ctx *c) {
    WbRanges rg;
    for (auto &r : rg.r) r = {0, c->cx * 8 - 1, 0, c->cy * 8 - 1, 0, c->cz * 8 - 1};
    return rg;
}
int wb_events(vxpt_ctx *c) {
    if (c->worldWritten) return 0;
    HIPCHK(c, hipEventCreateWithFlags(&c->worldWritten, hipEventDisableTiming));
    for (auto &e : c->editDone) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : c->wbEv) HIPCHK(c, hipEventCreate(&e));
    return 0;
}
// behind a build's / edit's kernels on the context stream: every earlier first half has finished before
// the stream got to them (its second half, which waited for it, was enqueued on this stream); the
// passes' first halves read the tables on the front streams, so those wait here
int wb_publish(vxpt_ctx *c) {
    HIPCHK(c, hipEventRecord(c->wbEv[1], c->stream));
    c->wbTimed = true;
    HIPCHK(c, hipEventRecord(c->worldWritten, c->stream));
    for (hipStream_t fs : c->frontStreams)
        if (fs) HIPCHK(c, hipStreamWaitEvent(fs, c->worldWritten, 0));
    return 0;
}

// every table of the ids on the device (c->voxels) by the kernels, enqueued on the context stream
int device_build_enqueue(vxpt_ctx *c) {
    const int BX = c->cx * 8, BY = c->cy * 8, BZ = c->cz * 8;
    const size_t nB = (size_t)BX * BY * BZ;
    if (nB > (size_t)INT_MAX) return fail(c, VXPT_ERR_ARG, "world too large");
    if (int r = wb_events(c)) return r;
    c->hOd = {};
    c->hBox = {};
    c->brickPrefix = BrickPrefix{};
    c->hSkyTop = {};
    if (grow(c, c->bricks, nB * 64) || grow(c, c->macro, nB / 64) || grow(c, c->cellMask, nB) ||
        grow(c, c->bdist, 8 * nB) || (c->useBoxes && grow(c, c->bbox, 8 * nB)) ||
        grow(c, c->skyTop, (size_t)4 * BX * BZ) || grow(c, c->dColTop, (size_t)BX * BZ) ||
        grow(c, c->dPrefix, wb::prefix_size(BX, BY, BZ)))
        return VXPT_ERR_HIP;
    c->nBricks = (int)nB;
    const WbWorld w = wb_world(c);
    HIPCHK(c, hipEventRecord(c->wbEv[0], c->stream));
    HIPCHK(c, launch_wb_occupancy(w, c->stream));
    HIPCHK(c, launch_wb_prefix(w, c->stream));
    HIPCHK(c, launch_wb_tables(w, wb_whole(c), c->stream));
    HIPCHK(c, launch_wb_sky_top(w, c->stream));
    return wb_publish(c);
}
// the same for uploaded ids, waited for; the host mirrors are built already
int device_build(vxpt_ctx *c) {
    if (int r = device_build_enqueue(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// A world whose ids were written on the device (c->voxels, c->cx / cy / cz set): the tables as
// device_build_enqueue, then the host mirrors build_mirrors would give for the same ids, read back
// instead of rebuilt.  The device holds the ids in both layouts, the cell and macro masks and the column
// tops already; k_terrain_mirrors adds the two counts.  One wait, behind the copies; `tables` and `read`
// are recorded behind the kernels and behind the copies.
int device_build_readback(vxpt_ctx *c, hipEvent_t tables, hipEvent_t read) {
    if (int r = device_build_enqueue(c)) return r;
    const int wx = c->cx * 32, wy = c->cy * 32, wz = c->cz * 32;
    const size_t nB = (size_t)c->nBricks, nCol = (size_t)(wx >> 2) * (wz >> 2);
    const int tx = (wx + 63) / 64, ty = (wy + 63) / 64, tz = (wz + 63) / 64;
    const size_t nTop = (size_t)tx * ty * tz;
    if (grow(c, c->dNonAir, nB) || grow(c, c->dTopCount, nTop)) return VXPT_ERR_HIP;
    hipStream_t st = c->stream;
    HIPCHK(c, launch_terrain_mirrors(wb_world(c), c->dNonAir.p, c->dTopCount.p, st));
    HIPCHK(c, hipEventRecord(tables, st));
    c->hIds.resize(nB * 64);
    c->hBricks.resize(nB * 64);
    c->hCell.resize(nB);
    c->hMacro.resize(nB / 64);
    c->hNonAir.resize(nB);
    c->topCount.resize(nTop);
    std::vector<uint32_t> col(nCol);
    HIPCHK(c, hipMemcpyAsync(c->hIds.data(), c->voxels.p, nB * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(c->hBricks.data(), c->bricks.p, nB * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(c->hCell.data(), c->cellMask.p, nB * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(c->hMacro.data(), c->macro.p, nB / 64 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(c->hNonAir.data(), c->dNonAir.p, nB, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(c->topCount.data(), c->dTopCount.p, nTop * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(col.data(), c->dColTop.p, nCol * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipEventRecord(read, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->colTop.assign(col.begin(), col.end());
    c->topValid = (nTop <= 64) ? 1 : 0;
    refresh_top(c);
    return 0;
}

}  // namespace

namespace vx::host {

// the cube and box tables of the current world, whole (a box switch or cap change)
int device_tables(vxpt_ctx *c) {
    if (c->useBoxes && grow(c, c->bbox, (size_t)8 * c->nBricks)) return VXPT_ERR_HIP;
    HIPCHK(c, hipEventRecord(c->wbEv[0], c->stream));
    HIPCHK(c, launch_wb_tables(wb_world(c), wb_whole(c), c->stream));
    if (int r = wb_publish(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace vx::host

namespace {

// what a batch of edits touched, for its one scatter: the cells (chunk-major and brick-major byte
// index; may repeat), the bricks whose cube mask changed with their occupancy before the batch, and
// the raised columns
struct EditBatch {
    std::vector<std::pair<size_t, size_t>> cells;
    std::map<size_t, bool> brickWas;
    std::map<size_t, std::array<int, 3>> brickAt;
    std::vector<size_t> cols;
    bool any = false;
};

// set_block's changes of the host mirrors (the position is valid), recorded in the batch
void edit_mirrors(vxpt_ctx *c, int x, int y, int z, int id, EditBatch &B) {
    const int wx = c->cx * 32;
    const size_t ci = (size_t)((x >> 5) + c->cx * ((z >> 5) + c->cz * (y >> 5))) * 32768 + (x & 31) +
                      32 * ((z & 31) + 32 * (y & 31));
    const int old = c->hIds[ci];
    if (old == id) return;
    B.any = true;
    c->hIds[ci] = (uint8_t)id;
    ++c->worldVersion;
    const size_t b = brick_lin(c, x >> 2, y >> 2, z >> 2);
    const int lc = (x & 3) + 4 * ((z & 3) + 4 * (y & 3));
    c->hBricks[b * 64 + lc] = (uint8_t)id;
    c->hNonAir[b] += (id != 0 ? 1 : 0) - (old != 0 ? 1 : 0);
    B.cells.emplace_back(ci, b * 64 + lc);
    if (is_cube(old) == is_cube(id)) return;
    const uint64_t before = c->hCell[b];
    if (B.brickWas.emplace(b, before != 0).second) B.brickAt[b] = {x >> 2, y >> 2, z >> 2};
    c->hCell[b] = is_cube(id) ? (before | (1ull << lc)) : (before & ~(1ull << lc));
    c->topCount[top_block(c, x, y, z)] += is_cube(id) ? 1 : -1;
    const size_t col = (size_t)(z >> 2) * (wx >> 2) + (x >> 2);
    if (is_cube(id) && c->colTop[col] < y + 1) {  // raised, never lowered: a bound
        c->colTop[col] = (uint16_t)(y + 1);
        B.cols.push_back(col);
    }
    if ((before != 0) != (c->hCell[b] != 0)) {
        const size_t m = b / 64;
        c->hMacro[m] = c->hCell[b] ? (c->hMacro[m] | (1ull << (b % 64))) : (c->hMacro[m] & ~(1ull << (b % 64)));
    }
}

// the batch onto the device, without waiting for it: the records through a pinned staging buffer, one
// scatter, and -- after an occupancy flip -- the prefix counts whole and the tables of, per octant, the
// bricks behind the flipped ones (their bounding range: set_block's region for one brick)
int edit_flush(vxpt_ctx *c, EditBatch &B) {
    if (!B.any) return 0;
    refresh_top(c);
    c->prevSceneEmpty = 1;
    std::sort(B.cells.begin(), B.cells.end());
    B.cells.erase(std::unique(B.cells.begin(), B.cells.end()), B.cells.end());
    std::sort(B.cols.begin(), B.cols.end());
    B.cols.erase(std::unique(B.cols.begin(), B.cols.end()), B.cols.end());
    const int BX = c->cx * 8, BY = c->cy * 8, BZ = c->cz * 8;
    std::set<size_t> macros;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
    for (const auto &kv : B.brickWas)
        if (kv.second != (c->hCell[kv.first] != 0)) {
            macros.insert(kv.first / 64);
            const auto &at = B.brickAt[kv.first];
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], at[a]);
                hi[a] = std::max(hi[a], at[a]);
            }
        }
    WbEditCounts cnt{{(uint32_t)B.cells.size(), (uint32_t)B.cells.size(), (uint32_t)B.brickWas.size(),
                      (uint32_t)macros.size(), (uint32_t)B.cols.size()}};
    const size_t total = 2 * B.cells.size() + B.brickWas.size() + macros.size() + B.cols.size();
    const int k = c->editNext;
    c->editNext ^= 1;
    // the kernel that read this buffer two batches ago has normally long finished
    if (c->editUsed[k]) HIPCHK(c, hipEventSynchronize(c->editDone[k]));
    if (c->editCap[k] < total) {
        if (c->editStage[k]) HIPCHK(c, hipHostFree(c->editStage[k]));
        c->editStage[k] = nullptr;
        c->editCap[k] = std::max<size_t>(1024, 2 * total);
        HIPCHK(c, hipHostMalloc((void **)&c->editStage[k], c->editCap[k] * sizeof(WbRec), hipHostMallocDefault));
    }
    WbRec *r = c->editStage[k];
    for (const auto &p : B.cells) *r++ = {p.first, c->hIds[p.first]};
    for (const auto &p : B.cells) *r++ = {p.second, c->hBricks[p.second]};
    for (const auto &kv : B.brickWas) *r++ = {kv.first, c->hCell[kv.first]};
    for (size_t m : macros) *r++ = {m, c->hMacro[m]};
    for (size_t col : B.cols) *r++ = {col, c->colTop[col]};
    const WbWorld w = wb_world(c);
    HIPCHK(c, hipEventRecord(c->wbEv[0], c->stream));
    HIPCHK(c, launch_wb_edit(w, c->editStage[k], cnt, c->stream));
    HIPCHK(c, hipEventRecord(c->editDone[k], c->stream));
    c->editUsed[k] = true;
    if (hi[0] >= 0) {
        HIPCHK(c, launch_wb_prefix(w, c->stream));
        WbRanges rg;
        for (int oct = 0; oct < 8; ++oct)
            rg.r[oct] = {(oct & 1) ? 0 : lo[0], (oct & 1) ? hi[0] : BX - 1, (oct & 2) ? 0 : lo[1],
                         (oct & 2) ? hi[1] : BY - 1, (oct & 4) ? 0 : lo[2], (oct & 4) ? hi[2] : BZ - 1};
        HIPCHK(c, launch_wb_tables(w, rg, c->stream));
    }
    if (!B.cols.empty()) HIPCHK(c, launch_wb_sky_top(w, c->stream));
    return wb_publish(c);
}

}  // namespace

namespace vx::host {

int world_from_device(vxpt_ctx *c, hipEvent_t tables, hipEvent_t read) { return device_build_readback(c, tables, read); }

// A lower bound on the distance from p to any primary hit: the nearest non-air cell's box, grown by
// meshGrow cells on every side (instanced meshes may overhang their cell; 1 unless a loaded mesh
// reaches further), over the host mirror of the world, within 64 cells of p's cell (beyond that,
// 63 - grow is the bound).  Empty space outside the world holds no geometry.  The search walks
// Chebyshev rings of 4^3 bricks around p's brick, visits the cells of non-empty bricks only
// (hNonAir) and stops once a ring cannot hold anything closer.
float nearest_surface(const vxpt_ctx *c, V3 p) {
    const int WX = c->cx * 32, WY = c->cy * 32, WZ = c->cz * 32;
    if (c->hIds.empty() || WX == 0 || c->hNonAir.empty()) return 1e30f;
    constexpr int kRings = 64;
    const float grow = c->meshGrow;
    const float cap = (float)(kRings - 1) - grow;
    auto gap = [&](float v, float lo, float hi) { return v < lo ? lo - v : (v > hi ? v - hi : 0.0f); };
    const int px = (int)std::floor(p.x), py = (int)std::floor(p.y), pz = (int)std::floor(p.z);
    const int bx0 = px >> 2, by0 = py >> 2, bz0 = pz >> 2;  // (arithmetic shift: floor for negatives)
    const int BX = WX / 4, BY = WY / 4, BZ = WZ / 4;
    float best = 1e30f;
    auto brick = [&](int bx, int by, int bz) {
        if (bx < 0 || by < 0 || bz < 0 || bx >= BX || by >= BY || bz >= BZ) return;
        const size_t b = brick_lin(c, bx, by, bz);
        if (!c->hNonAir[b]) return;
        const float dx = gap(p.x, 4.0f * bx - grow, 4.0f * bx + 4.0f + grow);
        const float dy = gap(p.y, 4.0f * by - grow, 4.0f * by + 4.0f + grow);
        const float dz = gap(p.z, 4.0f * bz - grow, 4.0f * bz + 4.0f + grow);
        if (std::sqrt(dx * dx + dy * dy + dz * dz) >= best) return;
        for (int lc = 0; lc < 64; ++lc) {
            if (!c->hBricks[b * 64 + lc]) continue;
            const int x = bx * 4 + (lc & 3), z = bz * 4 + ((lc >> 2) & 3), y = by * 4 + (lc >> 4);
            const float ex = gap(p.x, (float)x - grow, (float)(x + 1) + grow);
            const float ey = gap(p.y, (float)y - grow, (float)(y + 1) + grow);
            const float ez = gap(p.z, (float)z - grow, (float)(z + 1) + grow);
            best = std::min(best, std::sqrt(ex * ex + ey * ey + ez * ez));
        }
    };
    // cells within Chebyshev distance 64 of p's cell lie within 17 bricks of p's brick; a cell
    // further out is >= 64 - grow away, past the cap
    for (int r = 0; r <= kRings / 4 + 1; ++r) {
        // every brick of ring r is at least 4 (r - 1) - grow away along its farthest axis
        if (best <= 4.0f * (float)(r - 1) - grow) break;
        for (int dy = -r; dy <= r; ++dy)
            for (int dz = -r; dz <= r; ++dz) {
                const bool face = dy == -r || dy == r || dz == -r || dz == r;
                if (face) {
                    for (int dx = -r; dx <= r; ++dx) brick(bx0 + dx, by0 + dy, bz0 + dz);
                } else {
                    brick(bx0 - r, by0 + dy, bz0 + dz);
                    if (r > 0) brick(bx0 + r, by0 + dy, bz0 + dz);
                }
            }
    }
    return std::min(best, cap);
}

}  // namespace vx::host

extern "C" {

int vxpt_generate_terrain(vxpt_ctx *c, int cxn, int cyn, int czn, float heightScale, float freqDen, int flags) {
    if (!c || cxn <= 0 || cyn <= 0 || czn <= 0) return VXPT_ERR_ARG;
    const bool keepBalls = (flags & VXPT_TERRAIN_SHADER_BALLS) != 0, globalY = (flags & VXPT_TERRAIN_GLOBAL_Y) != 0;
    std::vector<uint8_t> ids((size_t)cxn * cyn * czn * 32768, 0);
    uint8_t perm[256];
    ter::permutation(124, perm);  // PerlinNoiseGenerator(4, 124), VoxelSceneGen.cu:361
    ter::generate_host(ter::Window{cxn, cyn, czn, 0, 0, 0, 1.0f / freqDen, heightScale, keepBalls, globalY}, perm, ids.data());
    return vxpt_upload_voxels(c, ids.data(), cxn, cyn, czn);
}

int vxpt_upload_voxels(vxpt_ctx *c, const uint8_t *ids, int cxn, int cyn, int czn) {
    if (!c || !ids || cxn <= 0 || cyn <= 0 || czn <= 0) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    c->cx = cxn; c->cy = cyn; c->cz = czn;
    const size_t n = (size_t)cxn * cyn * czn * 32768;
    c->hIds.assign(ids, ids + n);
    ++c->worldVersion;
    if (int r = upload_vec(c, c->voxels, c->hIds.data(), n)) return r;
    if (c->worldBuild == VXPT_WORLD_BUILD_DEVICE) {  // only the chunk-major ids cross to the device
        build_mirrors(c, c->hIds.data());
        if (int r = device_build(c)) return r;
    } else if (int r = build_occupancy(c, c->hIds.data())) {
        return r;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return refresh_instances(c, true, true);
}

int vxpt_upload_materials(vxpt_ctx *c, const vxpt_material *m, int n) {
    if (!c || !m || n < 1 || n >= kBlockTypes) return VXPT_ERR_ARG;
    for (int b = 1; b <= n; ++b) {
        const vxpt_material &s = m[b - 1];
        const MatDev old = c->mats[b];
        c->mats[b] = MatDev{{s.albedo[0], s.albedo[1], s.albedo[2]}, s.roughness, s.translucency, s.metallic,
                            s.material_id, s.thinfilm};
        if (b > 12) {  // instanced blocks keep their emissive / world-grid set-up (vxpt_load_models)
            c->mats[b].emissive = old.emissive;
            c->mats[b].worldGridUV = old.worldGridUV;
            c->mats[b].uvScale = old.uvScale;
        }
    }
    return VXPT_OK;
}

// VoxelEngine::performRayTraversal (VoxelEngine.cu:1040-1166): a unit-step walk of the camera
// ray over the host grid; the last empty cell before the first non-empty one is where a block
// would be placed.  out: hit, hit x, y, z, hit id, has space, place x, y, z, cells walked
int vxpt_pick_block(vxpt_ctx *c, int32_t out[10]) {
    if (!c || !out) return VXPT_ERR_ARG;
    if (c->hIds.empty()) return fail(c, VXPT_ERR_STATE, "no voxels uploaded");
    for (int i = 0; i < 10; ++i) out[i] = 0;
    const int W = c->cx * 32, H = c->cy * 32, D = c->cz * 32;
    const V3 o = c->cam.pos;
    V3 d = c->cam.dir;
    const float len = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
    if (len <= 1e-8f) return VXPT_OK;
    d = V3(d.x / len, d.y / len, d.z / len);
    int x = (int)std::floor(o.x), y = (int)std::floor(o.y), z = (int)std::floor(o.z);
    const int stx = d.x > 0.0f ? 1 : -1, sty = d.y > 0.0f ? 1 : -1, stz = d.z > 0.0f ? 1 : -1;
    auto delta = [](float v) { return std::fabs(v) < 1e-8f ? FLT_MAX : 1.0f / std::fabs(v); };
    auto first = [](float v, int cell, int step, float orig) {
        const float bound = step > 0 ? (float)(cell + 1) : (float)cell;
        return std::fabs(v) < 1e-8f ? FLT_MAX : (bound - orig) / v;
    };
    const float tdx = delta(d.x), tdy = delta(d.y), tdz = delta(d.z);
    float tmx = first(d.x, x, stx, o.x), tmy = first(d.y, y, sty, o.y), tmz = first(d.z, z, stz, o.z);
    int n = 0;
    while (n++ < 1000) {
        if (x < 0 || x >= W || y < 0 || y >= H || z < 0 || z >= D) break;
        const int id = c->hIds[(size_t)((x >> 5) + c->cx * ((z >> 5) + c->cz * (y >> 5))) * 32768 + (x & 31) +
                                32 * ((z & 31) + 32 * (y & 31))];
        if (id == 0) {
            out[5] = 1; out[6] = x; out[7] = y; out[8] = z;
        } else {
            out[0] = 1; out[1] = x; out[2] = y; out[3] = z; out[4] = id;
            break;
        }
        if (tmx < tmy) {
            if (tmx < tmz) { x += stx; tmx += tdx; }
            else { z += stz; tmz += tdz; }
        } else {
            if (tmy < tmz) { y += sty; tmy += tdy; }
            else { z += stz; tmz += tdz; }
        }
    }
    out[9] = n;
    return VXPT_OK;
}

static int id_at(const vxpt_ctx *c, int x, int y, int z) {
    const size_t ch = (size_t)(x >> 5) + (size_t)c->cx * ((z >> 5) + (size_t)c->cz * (y >> 5));
    return c->hIds[ch * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))];
}

int vxpt_set_block(vxpt_ctx *c, int x, int y, int z, int block_id) {
    if (!c) return VXPT_ERR_ARG;
    if (c->hIds.empty()) return fail(c, VXPT_ERR_STATE, "no voxels uploaded");
    if (c->worldBuild == VXPT_WORLD_BUILD_DEVICE) {  // a batch of one
        const int32_t e[4] = {x, y, z, block_id};
        return vxpt_set_blocks(c, e, 1);
    }
    HIPCHK(c, hipSetDevice(c->dev));
    int old = 0;
    if (x >= 0 && y >= 0 && z >= 0 && x < c->cx * 32 && y < c->cy * 32 && z < c->cz * 32) old = id_at(c, x, y, z);
    if (int r = set_block(c, x, y, z, block_id)) return r;
    return edit_instances(c, x, y, z, old, block_id);
}

int vxpt_set_blocks(vxpt_ctx *c, const int32_t *e, int n) {
    if (!c || n < 0 || (n > 0 && !e)) return VXPT_ERR_ARG;
    if (c->hIds.empty()) return fail(c, VXPT_ERR_STATE, "no voxels uploaded");
    for (int i = 0; i < n; ++i) {  // the whole batch before anything changes
        const int32_t *q = e + 4 * (size_t)i;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[0] >= c->cx * 32 || q[1] >= c->cy * 32 || q[2] >= c->cz * 32 ||
            q[3] < 0 || q[3] > 255)
            return fail(c, VXPT_ERR_ARG, "block position or id out of range");
    }
    // device instance mode: the edits' device work once, from the state after the last edit
    const bool outer = c->instBatch;
    c->instBatch = true;
    int rc = VXPT_OK;
    if (c->worldBuild != VXPT_WORLD_BUILD_DEVICE) {
        for (int i = 0; i < n && rc == VXPT_OK; ++i)
            rc = vxpt_set_block(c, e[4 * (size_t)i], e[4 * (size_t)i + 1], e[4 * (size_t)i + 2], e[4 * (size_t)i + 3]);
        c->instBatch = outer;
        if (!outer)
            if (int r = inst_flush(c)) return r;
        return rc;
    }
    if (hipSetDevice(c->dev) != hipSuccess) {
        c->instBatch = outer;
        return fail(c, VXPT_ERR_HIP, "hipSetDevice");
    }
    EditBatch B;
    for (int i = 0; i < n && rc == VXPT_OK; ++i) {
        const int32_t *q = e + 4 * (size_t)i;
        const int old = id_at(c, q[0], q[1], q[2]);
        edit_mirrors(c, q[0], q[1], q[2], q[3], B);
        rc = edit_instances(c, q[0], q[1], q[2], old, q[3]);
    }
    c->instBatch = outer;
    if (int r = edit_flush(c, B)) return r;
    if (!outer)
        if (int r = inst_flush(c)) return r;
    return rc;
}

int vxpt_set_world_build(vxpt_ctx *c, int mode) {
    if (!c || (mode != VXPT_WORLD_BUILD_HOST && mode != VXPT_WORLD_BUILD_DEVICE)) return VXPT_ERR_ARG;
    if (mode == c->worldBuild) return VXPT_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    for (hipStream_t fs : c->frontStreams) HIPCHK(c, hipStreamSynchronize(fs));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->worldBuild = mode;
    if (c->hIds.empty()) return VXPT_OK;
    // the loaded world's tables, rebuilt whole in the new mode
    ++c->worldVersion;
    if (mode == VXPT_WORLD_BUILD_DEVICE) {
        build_mirrors(c, c->hIds.data());
        return device_build(c);
    }
    return build_occupancy(c, c->hIds.data());
}

int vxpt_world_build_ms(vxpt_ctx *c, float *ms) {
    if (!c || !ms) return VXPT_ERR_ARG;
    if (!c->wbTimed) return fail(c, VXPT_ERR_STATE, "no device build or edit yet");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipEventSynchronize(c->wbEv[1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->wbEv[0], c->wbEv[1]));
    return VXPT_OK;
}

int vxpt_world_tables_host(const uint8_t *ids, int cx, int cy, int cz, int box_cap, int box_cap_up, uint8_t *brick_ids,
                           uint64_t *cell_masks, uint64_t *macro_masks, uint8_t *octant_tables, uint32_t *box_tables,
                           uint16_t *sky_top) {
    if (!ids || cx <= 0 || cy <= 0 || cz <= 0 || box_cap < 1 || box_cap > 255 || box_cap_up < 1 || box_cap_up > 255 ||
        (size_t)cx * 8 * cy * 8 * cz * 8 > (size_t)INT_MAX)
        return VXPT_ERR_ARG;
    wb::tables_host(ids, cx, cy, cz, box_cap, box_cap_up, brick_ids, cell_masks, macro_masks, octant_tables, box_tables,
                    sky_top);
    return VXPT_OK;
}

// VoxelEngine::update's click (VoxelEngine.cu:906-975): block 0 deletes the picked block,
// another id is placed in the last empty cell before it.  out = the pick (vxpt_pick_block)
int vxpt_click_block(vxpt_ctx *c, int block_id, int32_t out[10]) {
    int32_t pk[10];
    if (int r = vxpt_pick_block(c, pk)) return r;
    if (out) std::memcpy(out, pk, sizeof(pk));
    if (block_id == 0) {
        if (pk[0]) return vxpt_set_block(c, pk[1], pk[2], pk[3], 0);
    } else if (pk[5] && pk[0]) {
        return vxpt_set_block(c, pk[6], pk[7], pk[8], block_id);
    }
    return VXPT_OK;
}

// WorldSceneManager chunk files (WorldSceneManager.cpp:240-307): each 32^3 chunk's bytes in
// <chunk_dir>/<FNV-1a 64 of the bytes, 16 hex digits>.bin; the scene yaml (SceneConfig.cpp:116-151)
// lists them under `chunks:` with the camera and `chunk_config`.
static std::string fnv1a_hex(const uint8_t *p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        h ^= (unsigned long long)p[i];
        h *= 1099511628211ull;
    }
    char buf[17];
    std::snprintf(buf, sizeof buf, "%016llx", h);
    return buf;
}

int vxpt_save_world(vxpt_ctx *c, const char *scene_yaml, const char *chunk_dir) {
    if (!c || !scene_yaml || !chunk_dir) return VXPT_ERR_ARG;
    if (c->hIds.empty()) return fail(c, VXPT_ERR_STATE, "no voxels uploaded");
    std::error_code ec;
    std::filesystem::create_directories(chunk_dir, ec);
    const int nch = c->cx * c->cy * c->cz;
    std::vector<std::string> hashes(nch);
    for (int i = 0; i < nch; ++i) {
        const uint8_t *d = c->hIds.data() + (size_t)i * 32768;
        hashes[i] = fnv1a_hex(d, 32768);
        std::ofstream f(std::filesystem::path(chunk_dir) / (hashes[i] + ".bin"), std::ios::binary | std::ios::trunc);
        f.write((const char *)d, 32768);
        if (!f.good()) return fail(c, VXPT_ERR_IO, "cannot write chunk " + std::to_string(i));
    }
    std::ofstream y(scene_yaml, std::ios::trunc);
    if (!y) return fail(c, VXPT_ERR_IO, std::string("cannot write ") + scene_yaml);
    auto f3 = [](V3 v) {
        std::ostringstream o;
        o << "[" << v.x << ", " << v.y << ", " << v.z << "]";
        return o.str();
    };
    y << "# Scene Configuration File\n# Generated automatically\n\n"
      << "camera:\n  position: " << f3(c->cam.pos) << "\n  direction: " << f3(c->cam.dir)
      << "\n  up: " << f3(V3(0.0f, 1.0f, 0.0f)) << "\n  fov: " << 90.0f << "\n\n"
      << "character:\n  position: " << f3(V3(16.0f, 10.0f, 16.0f)) << "\n  rotation: " << f3(V3(0.0f))
      << "\n  scale: " << f3(V3(1.0f)) << "\n"
      << "\nchunk_config:\n  chunksX: " << c->cx << "\n  chunksY: " << c->cy << "\n  chunksZ: " << c->cz << "\n"
      << "\nchunks:\n";
    for (int i = 0; i < nch; ++i) y << "  " << i << ": " << hashes[i] << "\n";
    return y.good() ? VXPT_OK : fail(c, VXPT_ERR_IO, "scene yaml write failed");
}

// WorldSceneManager::LoadScene (:365-458): the camera and every listed chunk file; a world of
// another chunk configuration keeps the runtime one (records past it are errors), and without a
// world yet the scene's configuration is used.  The world is then rebuilt (VoxelEngine::reload).
int vxpt_load_world(vxpt_ctx *c, const char *scene_yaml, const char *chunk_dir, vxpt_camera *cam_out) {
    if (!c || !scene_yaml || !chunk_dir) return VXPT_ERR_ARG;
    std::ifstream f(scene_yaml);
    if (!f) return fail(c, VXPT_ERR_IO, std::string("cannot open ") + scene_yaml);
    std::string line, section;
    int cfg[3] = {0, 0, 0};
    std::vector<std::pair<int, std::string>> recs;
    while (std::getline(f, line)) {
        line = trim(line);
        if (line.empty() || line[0] == '#') continue;
        if (line.back() == ':') { section = line.substr(0, line.size() - 1); continue; }
        const size_t col = line.find(':');
        if (col == std::string::npos) continue;
        const std::string key = trim(line.substr(0, col)), val = trim(line.substr(col + 1));
        if (section == "chunk_config") {
            if (key == "chunksX") cfg[0] = std::atoi(val.c_str());
            else if (key == "chunksY") cfg[1] = std::atoi(val.c_str());
            else if (key == "chunksZ") cfg[2] = std::atoi(val.c_str());
        } else if (section == "chunks" && !key.empty() && std::isdigit((unsigned char)key[0])) {
            recs.emplace_back(std::atoi(key.c_str()), val);
        }
    }
    if (cam_out && vxpt_load_scene_camera(c, scene_yaml, cam_out) != VXPT_OK) return VXPT_ERR_IO;
    if (c->hIds.empty()) {
        if (cfg[0] <= 0 || cfg[1] <= 0 || cfg[2] <= 0) return fail(c, VXPT_ERR_STATE, "no world and no chunk_config");
        c->cx = cfg[0]; c->cy = cfg[1]; c->cz = cfg[2];
        c->hIds.assign((size_t)c->cx * c->cy * c->cz * 32768, 0);
    }
    const int nch = c->cx * c->cy * c->cz;
    std::vector<uint8_t> ids = c->hIds;
    bool ok = true;
    for (const auto &r : recs) {
        if (r.first < 0 || r.first >= nch) { ok = false; continue; }
        const auto path = std::filesystem::path(chunk_dir) / (r.second + ".bin");
        std::error_code ec;
        if (std::filesystem::file_size(path, ec) != 32768 || ec) { ok = false; continue; }
        std::ifstream in(path, std::ios::binary);
        in.read((char *)ids.data() + (size_t)r.first * 32768, 32768);
        if (in.gcount() != 32768) ok = false;
    }
    if (int r = vxpt_upload_voxels(c, ids.data(), c->cx, c->cy, c->cz)) return r;
    return ok ? VXPT_OK : fail(c, VXPT_ERR_IO, "some chunk records could not be loaded");
}

int vxpt_nearest_surface(vxpt_ctx *c, const float pos[3], float *dist) {
    if (!c || !pos || !dist) return VXPT_ERR_ARG;
    *dist = nearest_surface(c, V3(pos[0], pos[1], pos[2]));
    return VXPT_OK;
}

}  // extern "C"
