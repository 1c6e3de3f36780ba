// vxpt -- host runtime, the terrain with an origin and a seed: the argument checks, the host
// generator behind vxpt_terrain_host, and the device path of vxpt_generate_terrain_ex (terrain.hip's
// kernels, then the world's tables and host mirrors from what the device holds: host_world.cpp).
#include <cmath>
#include <cstdint>
#include <vector>

#include "host_ctx.hpp"
#include "terrain.hpp"

namespace {

// the generator's window of a descriptor; false: VXPT_ERR_ARG
bool terrain_window(const vxpt_terrain_desc *d, ter::Window &w) {
    if (!d || d->chunks[0] <= 0 || d->chunks[1] <= 0 || d->chunks[2] <= 0 || d->freq_den == 0.0f) return false;
    const bool globalY = (d->flags & VXPT_TERRAIN_GLOBAL_Y) != 0;
    if (!globalY && d->origin[1] != 0) return false;
    // every compared coordinate converts to float exactly
    for (int a = 0; a < 3; ++a) {
        const int64_t lo = d->origin[a], hi = lo + (int64_t)d->chunks[a] * 32, lim = 1 << 24;
        if (lo <= -lim || lo >= lim || hi <= -lim || hi >= lim) return false;
    }
    // the brick count is an int (as vxpt_world_tables_host)
    if ((uint64_t)d->chunks[0] * (uint64_t)d->chunks[1] * (uint64_t)d->chunks[2] > (uint64_t)INT32_MAX / 512) return false;
    w = ter::Window{d->chunks[0], d->chunks[1], d->chunks[2], d->origin[0], d->origin[1], d->origin[2],
                    1.0f / d->freq_den, d->height_scale, (d->flags & VXPT_TERRAIN_SHADER_BALLS) != 0, globalY};
    return true;
}

}  // namespace

int vxpt_terrain_host(const vxpt_terrain_desc *d, uint8_t *ids) {
    ter::Window w;
    if (!ids || !terrain_window(d, w)) return VXPT_ERR_ARG;
    uint8_t perm[256];
    ter::permutation(d->seed, perm);
    ter::generate_host(w, perm, ids);
    return VXPT_OK;
}

int vxpt_generate_terrain_ex(vxpt_ctx *c, const vxpt_terrain_desc *d) {
    ter::Window w;
    if (!c) return VXPT_ERR_ARG;
    if (!terrain_window(d, w)) return fail(c, VXPT_ERR_ARG, "terrain descriptor out of range");
    const size_t n = (size_t)w.cx * w.cy * w.cz * 32768;
    if (c->worldBuild != VXPT_WORLD_BUILD_DEVICE) {
        c->terTimed = false;
        std::vector<uint8_t> ids(n);
        if (int r = vxpt_terrain_host(d, ids.data())) return r;
        return vxpt_upload_voxels(c, ids.data(), w.cx, w.cy, w.cz);
    }
    HIPCHK(c, hipSetDevice(c->dev));
    for (auto &e : c->terEv)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (grow(c, c->terPerm, 256) || grow(c, c->terHeight, (size_t)w.cx * 32 * w.cz * 32) || grow(c, c->voxels, n))
        return VXPT_ERR_HIP;
    c->cx = w.cx; c->cy = w.cy; c->cz = w.cz;
    ++c->worldVersion;
    c->terTimed = false;
    // the table is all that crosses to the device (a pageable source: copied out before the call returns)
    uint8_t perm[256];
    ter::permutation(d->seed, perm);
    HIPCHK(c, hipMemcpyAsync(c->terPerm.p, perm, 256, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->terEv[0], c->stream));
    HIPCHK(c, launch_terrain_height(w, c->terPerm.p, c->terHeight.p, c->stream));
    HIPCHK(c, hipEventRecord(c->terEv[1], c->stream));
    HIPCHK(c, launch_terrain_fill(w, c->terHeight.p, c->voxels.p, c->stream));
    HIPCHK(c, hipEventRecord(c->terEv[2], c->stream));
    if (int r = world_from_device(c, c->terEv[3], c->terEv[4])) return r;
    c->terTimed = true;
    return refresh_instances(c, true, true);
}

int vxpt_terrain_ms(vxpt_ctx *c, float out[4]) {
    if (!c || !out) return VXPT_ERR_ARG;
    if (!c->terTimed) return fail(c, VXPT_ERR_STATE, "no terrain generated on the device yet");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipEventSynchronize(c->terEv[4]));
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipEventElapsedTime(&out[k], c->terEv[k], c->terEv[k + 1]));
    return VXPT_OK;
}
