// vxpt -- host runtime, instanced block meshes and their emissive-triangle lights: the instance set, BLAS and
// TLAS, light tables and light updates on the host or on the device (instances.hip), the mesh probes, models.yaml.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "bvh_build.hpp"
#include "host_ctx.hpp"
#include "lbvh.hpp"

namespace vx::host {

MeshDev mesh_dev(const vxpt_ctx *c) {
    return MeshDev{c->tlas.p, c->meshInst.p, c->blas.p, c->blasTri.p, c->blasTriId.p, c->blasRoot.p, c->nMeshInst};
}

}  // namespace vx::host

extern "C" {

// ---------------------------------------------------------------- instanced meshes + lights
namespace {

// VoxelEngine::collectInstanceTransforms (VoxelEngine.cu:323-384): for every instanced
// object (block 13..29 -> object id = block - 1), every cell holding the block -- or, for a
// light with a paired base, holding the base block -- is an instance of the object; a light
// cell also registers an instance of its base.  Instance id = PositionToInstanceId
// (VoxelMath.h:120-133: first instanced block + object * W^3 + x + W * (z + W * y), every
// coordinate clamped to W - 1, W = the world's x extent); ids are kept in a set per object
// (Scene.h:77) and a later cell with the same id overwrites the transform.
uint32_t instance_id(const vxpt_ctx *c, unsigned obj, unsigned x, unsigned y, unsigned z) {
    int first = kBlockTypes;
    for (int b = 0; b < kBlockTypes; ++b)
        if (c->blocks[b].instanced) { first = b; break; }
    const unsigned W = (unsigned)c->cx * 32u;
    x = x < W - 1 ? x : W - 1;
    y = y < W - 1 ? y : W - 1;
    z = z < W - 1 ? z : W - 1;
    return (unsigned)first + obj * W * W * W + (x + W * (z + W * y));
}

// what each block id contributes to the instance set: its own object; a base block also the objects
// of the lights paired with it; a paired light also its base's object
int instance_contrib(const vxpt_ctx *c, std::vector<int> contrib[kBlockTypes]) {
    int first = kBlockTypes;
    for (int b = 0; b < kBlockTypes; ++b)
        if (c->blocks[b].instanced) { first = b; break; }
    for (int obj = first - 1; obj < kBlockTypes - 1; ++obj) {
        const int block = obj + 1, base = c->blocks[block].lightBase;
        contrib[block].push_back(obj);
        if (base > 0 && base < kBlockTypes) {
            contrib[base].push_back(obj);
            contrib[block].push_back(base - 1);
        }
    }
    return first;
}

// the kept set as rows (objectId, instanceId, x, y, z), by object, then instance id
void flatten_instances(vxpt_ctx *c) {
    c->instances.clear();
    for (const auto &o : c->instSet)
        for (const auto &i : o.second)
            c->instances.insert(c->instances.end(),
                                {o.first, (int32_t)i.first, (int32_t)i.second[0], (int32_t)i.second[1], (int32_t)i.second[2]});
}

void collect_instances(vxpt_ctx *c) {
    c->instances.clear();
    c->instSet.clear();
    c->instSetValid = false;
    if (c->hIds.empty()) return;
    const unsigned W = (unsigned)c->cx * 32u, H = (unsigned)c->cy * 32u, D = (unsigned)c->cz * 32u;
    auto &byObject = c->instSet;
    auto inst_id = [&](unsigned obj, unsigned x, unsigned y, unsigned z) { return instance_id(c, obj, x, y, z); };
    // one pass over the cells
    std::vector<int> contrib[kBlockTypes];
    const int first = instance_contrib(c, contrib);
    for (unsigned x = 0; x < W; ++x)  // the reference's x, y, z order (last write wins)
        for (unsigned y = 0; y < H; ++y)
            for (unsigned z = 0; z < D; ++z) {
                const size_t ch = (x >> 5) + (size_t)c->cx * ((z >> 5) + (size_t)c->cz * (y >> 5));
                const int id = c->hIds[ch * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))];
                if (id < first || id >= kBlockTypes) continue;
                for (int obj : contrib[id]) byObject[obj][inst_id(obj, x, y, z)] = {x, y, z};
            }
    flatten_instances(c);
    // only device mode edits the set: host mode, which scans at every refresh, does not keep it
    if (c->instBuild == VXPT_INSTANCE_BUILD_DEVICE) c->instSetValid = true;
    else c->instSet.clear();
}

// One edit of the kept set (device instance mode), old id -> id at a valid cell, instead of the scan.
// In a cubic world every coordinate is below the clamp of instance_id, so an (object, cell) pair has
// its own id and a cell holds one block: the entry of each object the old id contributed goes, that
// of each object the new id contributes comes.  In a non-cubic world two cells can share an id (the
// scan's last write wins, which a local rule cannot reproduce): those worlds keep the scan.
void edit_instance_set(vxpt_ctx *c, int x, int y, int z, int old, int id) {
    if (!c->instSetValid || c->cx != c->cy || c->cx != c->cz) {
        collect_instances(c);
        return;
    }
    std::vector<int> contrib[kBlockTypes];
    const int first = instance_contrib(c, contrib);
    if (old >= first && old < kBlockTypes)
        for (int obj : contrib[old]) {
            const auto it = c->instSet.find(obj);
            if (it == c->instSet.end()) continue;
            it->second.erase(instance_id(c, (unsigned)obj, (unsigned)x, (unsigned)y, (unsigned)z));
            if (it->second.empty()) c->instSet.erase(it);
        }
    if (id >= first && id < kBlockTypes)
        for (int obj : contrib[id])
            c->instSet[obj][instance_id(c, (unsigned)obj, (unsigned)x, (unsigned)y, (unsigned)z)] = {(unsigned)x, (unsigned)y, (unsigned)z};
    flatten_instances(c);
}

// VoxelEngine::countLightTriangles / generateInstanceLights (VoxelEngine.cu:386-520) and
// buildAliasTable (:150-192): the emissive objects in object order, each instance's
// triangles in a row, one launch per object; then the weights' alias table (build_alias,
// the same construction as the sky's) and their sum (accumulatedLocalLightLuminance).
// the light table's layout from the instance rows: the light mapping and count, and (geometry) every
// emissive mesh's triangles, instance cells and runs; returns the light count
struct LightRun { size_t tri, cell; int nTri, nInst; V3 rad; };
size_t light_layout(vxpt_ctx *c, bool geometry, std::vector<float> &tri, std::vector<int> &cells,
                    std::vector<LightRun> &runs) {
    c->lightMap.clear();
    c->nLights = 0;
    size_t total = 0;
    for (size_t k = 0; k < c->instances.size(); k += 5) {
        const auto &bd = c->blocks[c->instances[k] + 1];
        if (bd.emissive) total += (size_t)bd.triangles;
    }
    if (total == 0) return 0;
    for (size_t k = 0; k < c->instances.size();) {
        const int obj = c->instances[k];
        const auto &bd = c->blocks[obj + 1];
        size_t e = k;
        while (e < c->instances.size() && c->instances[e] == obj) e += 5;
        if (bd.emissive && bd.triangles > 0) {
            LightRun r{tri.size(), cells.size(), bd.triangles, (int)((e - k) / 5),
                       V3(bd.emission[0], bd.emission[1], bd.emission[2])};
            if (geometry) tri.insert(tri.end(), bd.pos.begin(), bd.pos.end());
            for (size_t i = k; i < e; i += 5) {
                if (geometry) cells.insert(cells.end(), {c->instances[i + 2], c->instances[i + 3], c->instances[i + 4]});
                c->lightMap.insert(c->lightMap.end(),
                                   {(uint32_t)c->instances[i + 1], (uint32_t)c->nLights, (uint32_t)bd.triangles});
                c->nLights += (unsigned)bd.triangles;
            }
            runs.push_back(r);
        }
        k = e;
    }
    return total;
}

int build_lights(vxpt_ctx *c) {
    c->localLightLum = 0.0f;
    c->lightLumOnDevice = false;
    // all emissive meshes' triangles and instance cells, uploaded once
    std::vector<float> tri;
    std::vector<int> cells;
    std::vector<LightRun> runs;
    const size_t total = light_layout(c, true, tri, cells, runs);
    if (total == 0) return VXPT_OK;
    if (c->lights.n < total) {
        if (dalloc(c, c->lights.p, total)) return VXPT_ERR_HIP;
        c->lights.n = total;
    }
    if (c->lightWeight.n < total) {
        if (dalloc(c, c->lightWeight.p, total)) return VXPT_ERR_HIP;
        c->lightWeight.n = total;
    }
    if (int r = upload_vec(c, c->lightTri, tri.data(), tri.size())) return r;
    if (int r = upload_vec(c, c->lightInst, cells.data(), cells.size())) return r;
    size_t off = 0;
    for (const LightRun &r : runs) {
        HIPCHK(c, launch_tri_lights(c->lightTri.p + r.tri, r.nTri, c->lightInst.p + r.cell, r.nInst, r.rad,
                                    c->lights.p + off, c->lightWeight.p + off, c->stream));
        off += (size_t)r.nTri * r.nInst;
    }
    std::vector<float> w(total);
    HIPCHK(c, hipMemcpyAsync(w.data(), c->lightWeight.p, total * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const std::vector<AliasBin> bins = build_alias(w, c->localLightLum);
    if (int r = upload_vec(c, c->lightAlias, bins.data(), bins.size())) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ibStats[3] += 2;
    return VXPT_OK;
}

}  // namespace

// every loaded mesh's BLAS (object space), concatenated
int build_blas(vxpt_ctx *c) {
    c->hBlas.clear();
    c->hBlasTri.clear();
    c->hBlasUV.clear();
    c->hBlasTriId.clear();
    c->hRoot.assign(kBlockTypes, make_int2(-1, -1));
    for (int b = 0; b < kBlockTypes; ++b) {
        const auto &bd = c->blocks[b];
        if (!bd.instanced || bd.triangles == 0) continue;
        std::vector<float> box((size_t)bd.triangles * 6);
        for (int t = 0; t < bd.triangles; ++t)
            for (int k = 0; k < 3; ++k) {
                const float *v = &bd.pos[(size_t)t * 9];
                box[(size_t)t * 6 + k] = std::min(v[k], std::min(v[3 + k], v[6 + k]));
                box[(size_t)t * 6 + 3 + k] = std::max(v[k], std::max(v[3 + k], v[6 + k]));
            }
        std::vector<BvhNode> nodes;
        std::vector<int> order;
        int depth = 0;
        if (!build_bvh(box, 4, nodes, order, &depth)) return fail(c, VXPT_ERR_STATE, "mesh BVH too deep");
        c->hRoot[b] = make_int2((int)c->hBlas.size(), (int)c->hBlasTriId.size());
        c->hBlas.insert(c->hBlas.end(), nodes.begin(), nodes.end());
        for (int t : order) {
            c->hBlasTri.insert(c->hBlasTri.end(), bd.pos.begin() + (size_t)t * 9, bd.pos.begin() + (size_t)t * 9 + 9);
            c->hBlasUV.insert(c->hBlasUV.end(), bd.uv.begin() + (size_t)t * 6, bd.uv.begin() + (size_t)t * 6 + 6);
            c->hBlasTriId.push_back(t);
        }
    }
    if (!c->hBlas.empty()) {
        if (int r = upload_vec(c, c->blas, c->hBlas.data(), c->hBlas.size())) return r;
        if (int r = upload_vec(c, c->blasTri, c->hBlasTri.data(), c->hBlasTri.size())) return r;
        if (int r = upload_vec(c, c->blasUV, c->hBlasUV.data(), c->hBlasUV.size())) return r;
        if (int r = upload_vec(c, c->blasTriId, c->hBlasTriId.data(), c->hBlasTriId.size())) return r;
    }
    return upload_vec(c, c->blasRoot, c->hRoot.data(), c->hRoot.size());
}

// the world's TLAS over the instances whose block type has a mesh
int build_tlas(vxpt_ctx *c) {
    std::vector<MeshInst> mi;
    std::vector<float> box;
    for (size_t k = 0; k < c->instances.size(); k += 5) {
        const int block = c->instances[k] + 1;
        const int2 r = c->hRoot.empty() ? make_int2(-1, -1) : c->hRoot[block];
        if (r.x < 0) continue;
        const BvhNode &root = c->hBlas[r.x];
        const float cell[3] = {(float)c->instances[k + 2], (float)c->instances[k + 3], (float)c->instances[k + 4]};
        mi.push_back(MeshInst{{cell[0], cell[1], cell[2]}, block, (int)(k / 5)});
        for (int a = 0; a < 3; ++a) box.push_back(root.lo[a] + cell[a]);
        for (int a = 0; a < 3; ++a) box.push_back(root.hi[a] + cell[a]);
    }
    std::vector<BvhNode> nodes;
    std::vector<int> order;
    int depth = 0;
    if (!build_bvh(box, 2, nodes, order, &depth)) return fail(c, VXPT_ERR_STATE, "instance BVH too deep");
    std::vector<MeshInst> sorted;
    for (int i : order) sorted.push_back(mi[i]);
    c->nMeshInst = (int)sorted.size();
    c->nTlasNodes = c->nMeshInst ? (int)nodes.size() : 0;
    ++c->ibStats[1];
    if (c->nMeshInst == 0) return VXPT_OK;
    if (int r = upload_vec(c, c->tlas, nodes.data(), nodes.size())) return r;
    return upload_vec(c, c->meshInst, sorted.data(), sorted.size());
}

// VoxelEngine::updateLight (VoxelEngine.cu:658-709) after the light table was rebuilt from
// prevN lights: the remap table (light_map.hpp), uploaded for the next trace pass, which applies
// it to the previous reservoirs (Restir.h:48-79).
int light_update(vxpt_ctx *c, unsigned prevN) {
    const std::vector<int> remap = light_id_map(c->lightState, c->lightMap, prevN, c->nLights);
    if (prevN > 0) {
        if (int r = upload_vec(c, c->lightRemap, remap.data(), remap.size())) return r;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ++c->ibStats[3];
    }
    c->prevNumLights = prevN;
    c->lightsDirty = 1;
    return VXPT_OK;
}

// per instance row: cell + block, and its first light record (-1: not an emissive instance)
void instance_rows(const vxpt_ctx *c, std::vector<int4> &rows, std::vector<int> &rowLight) {
    const size_t n = c->instances.size() / 5;
    rows.resize(n);
    rowLight.assign(n, -1);
    std::map<uint32_t, int> firstLight;
    for (size_t k = 0; k < c->lightMap.size(); k += 3) firstLight[c->lightMap[k]] = (int)c->lightMap[k + 1];
    for (size_t i = 0; i < n; ++i) {
        const int32_t *r = &c->instances[i * 5];
        rows[i] = make_int4(r[2], r[3], r[4], r[0] + 1);
        // the light mapping is by instance id within the emissive object's run (closesthit.cu:869-899)
        const auto it = firstLight.find((uint32_t)r[1]);
        if (it != firstLight.end() && c->blocks[r[0] + 1].emissive) rowLight[i] = it->second;
    }
}

// device instance mode ------------------------------------------------------------------------------
// a pinned staging buffer of `bytes` that no enqueued copy still reads: one of the pool whose event has
// passed; while every one is busy the pool grows (to 8), and only then the host waits (counted)
int inst_stage(vxpt_ctx *c, size_t bytes, int &slot) {
    if (c->instStage.size() < 2) c->instStage.resize(2);
    slot = -1;
    for (size_t i = 0; i < c->instStage.size() && slot < 0; ++i)
        if (!c->instStage[i].used || hipEventQuery(c->instStage[i].done) == hipSuccess) slot = (int)i;
    (void)hipGetLastError();  // a pending event's hipErrorNotReady
    if (slot < 0 && c->instStage.size() < 8) {
        c->instStage.emplace_back();
        slot = (int)c->instStage.size() - 1;
    }
    if (slot < 0) {
        slot = 0;
        HIPCHK(c, hipEventSynchronize(c->instStage[0].done));
        ++c->ibStats[3];
    }
    auto &s = c->instStage[slot];
    if (!s.done) HIPCHK(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (s.cap < bytes) {
        if (s.p) HIPCHK(c, hipHostFree(s.p));
        s.p = nullptr;
        s.cap = std::max<size_t>(1 << 16, 2 * bytes);
        HIPCHK(c, hipHostMalloc((void **)&s.p, s.cap, hipHostMallocDefault));
    }
    return 0;
}

// What the edits since the last flush left to do on the device, from the host state as it is now, without
// waiting for the GPU: the rows, the TLAS (instances.hip) and -- after a light update -- the light
// records, their alias table (sky.hip's parallel construction) and the remap.  Enqueued on the context
// stream: every earlier first half has finished before the stream gets here (its second half, which
// waited for it, was enqueued on this stream); the passes' first halves read the tables on the front
// streams, so those wait for the event behind it.
int inst_flush(vxpt_ctx *c) {
    if (!c->instDirty) return VXPT_OK;
    const bool lights = c->instLightsDirty;
    if (lights && c->nLights > (unsigned)ab::kMaxN)  // the flags stay: the tables are not the state's
        return fail(c, VXPT_ERR_STATE, "too many lights for the device alias build");
    c->instDirty = c->instLightsDirty = false;
    ++c->ibStats[0];
    if (!c->instWritten) {
        HIPCHK(c, hipEventCreateWithFlags(&c->instWritten, hipEventDisableTiming));
        for (auto &e : c->ibEv) HIPCHK(c, hipEventCreate(&e));
    }
    std::vector<int4> rows;
    std::vector<int> rowLight, miRow;
    instance_rows(c, rows, rowLight);
    const size_t n = rows.size();
    for (size_t i = 0; i < n; ++i)
        if (!c->hRoot.empty() && c->hRoot[rows[i].w].x >= 0) miRow.push_back((int)i);
    const size_t nm = miRow.size();
    const bool onDevice = lbvh::world_fits(c->cx * 32, c->cy * 32, c->cz * 32);
    std::vector<float> tri;
    std::vector<int> cells;
    std::vector<LightRun> runs;
    size_t total = 0;
    if (lights) total = light_layout(c, true, tri, cells, runs);
    const bool remap = lights && c->prevNumLights > 0 && !c->hRemap.empty();
    // one staging block: rows, row lights, mesh rows, triangles, cells, remap (each 16-byte aligned)
    const auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t oRows = 0, oRowLight = oRows + al(n * 16), oMi = oRowLight + al(n * 4), oTri = oMi + al(nm * 4),
                 oCells = oTri + al(tri.size() * 4), oRemap = oCells + al(cells.size() * 4),
                 bytes = oRemap + al(remap ? c->hRemap.size() * 4 : 0);
    int slot = 0;
    if (int r = inst_stage(c, std::max<size_t>(bytes, 16), slot)) return r;
    char *st = c->instStage[slot].p;
    if (n) {
        std::memcpy(st + oRows, rows.data(), n * 16);
        std::memcpy(st + oRowLight, rowLight.data(), n * 4);
    }
    if (nm) std::memcpy(st + oMi, miRow.data(), nm * 4);
    if (!tri.empty()) std::memcpy(st + oTri, tri.data(), tri.size() * 4);
    if (!cells.empty()) std::memcpy(st + oCells, cells.data(), cells.size() * 4);
    if (remap) std::memcpy(st + oRemap, c->hRemap.data(), c->hRemap.size() * 4);
    if (grow2(c, c->meshRow, n) || grow2(c, c->meshRowLight, n) || grow2(c, c->lbMiRow, nm)) return VXPT_ERR_HIP;
    if (lights && total &&
        (grow2(c, c->lights, total) || grow2(c, c->lightWeight, total) || grow2(c, c->lightAlias, total) ||
         grow2(c, c->lightTri, tri.size()) || grow2(c, c->lightInst, cells.size())))
        return VXPT_ERR_HIP;
    if (remap && grow2(c, c->lightRemap, c->hRemap.size())) return VXPT_ERR_HIP;
    if (lights && total) {
        if (int r = alias_scratch(c, (int)total)) return r;
        if (!c->lightHead && dalloc(c, c->lightHead, 1)) return VXPT_ERR_HIP;
    }
    HIPCHK(c, hipEventRecord(c->ibEv[0], c->stream));
    const auto up = [&](void *dst, size_t off, size_t b) {
        return b ? hipMemcpyAsync(dst, st + off, b, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIPCHK(c, up(c->meshRow.p, oRows, n * 16));
    HIPCHK(c, up(c->meshRowLight.p, oRowLight, n * 4));
    HIPCHK(c, up(c->lbMiRow.p, oMi, nm * 4));
    if (nm == 0) {
        c->nMeshInst = 0;
        c->nTlasNodes = 0;
    } else if (onDevice) {
        if (grow2(c, c->tlas, 2 * nm - 1) || grow2(c, c->meshInst, nm) || grow2(c, c->lbPacked, (size_t)lbvh_padded((int)nm)) ||
            grow2(c, c->lbPrimBox, 6 * nm) || grow2(c, c->lbExact, 6 * (2 * nm - 1)) || grow2(c, c->lbSlotInner, nm) ||
            grow2(c, c->lbSlotLeaf, nm) || grow2(c, c->lbVisits, nm))
            return VXPT_ERR_HIP;
        const LbvhDev a{(int)nm, lbvh_padded((int)nm), c->lbMiRow.p, c->meshRow.p, c->blasRoot.p, c->blas.p,
                        c->lbPacked.p, c->lbPrimBox.p, c->lbExact.p, c->lbSlotInner.p, c->lbSlotLeaf.p, c->lbVisits.p,
                        c->tlas.p, c->meshInst.p};
        HIPCHK(c, launch_lbvh_build(a, c->stream));
        c->nMeshInst = (int)nm;
        c->nTlasNodes = 2 * (int)nm - 1;
        ++c->ibStats[1];
    } else {
        // more than 1024 cells on an axis: the host builder, whose uploads from pageable memory hold the
        // host until the copies are staged -- counted as a host wait
        if (int r = build_tlas(c)) return r;
        ++c->ibStats[3];
    }
    if (lights) {
        ++c->ibStats[2];
        c->localLightLum = 0.0f;
        c->lightLumOnDevice = total > 0;
        if (total) {
            HIPCHK(c, up(c->lightTri.p, oTri, tri.size() * 4));
            HIPCHK(c, up(c->lightInst.p, oCells, cells.size() * 4));
            size_t off = 0;
            for (const LightRun &r : runs) {
                HIPCHK(c, launch_tri_lights(c->lightTri.p + r.tri, r.nTri, c->lightInst.p + r.cell, r.nInst, r.rad,
                                            c->lights.p + off, c->lightWeight.p + off, c->stream));
                off += (size_t)r.nTri * r.nInst;
            }
            HIPCHK(c, launch_alias_build(c->lightWeight.p, (int)total, c->aliasScratch, c->lightHead, c->lightAlias.p,
                                         c->stream));
        }
        if (remap) HIPCHK(c, up(c->lightRemap.p, oRemap, c->hRemap.size() * 4));
    }
    HIPCHK(c, hipEventRecord(c->instStage[slot].done, c->stream));
    c->instStage[slot].used = true;
    HIPCHK(c, hipEventRecord(c->ibEv[1], c->stream));
    c->ibTimed = true;
    HIPCHK(c, hipEventRecord(c->instWritten, c->stream));
    for (hipStream_t fs : c->frontStreams)
        if (fs) HIPCHK(c, hipStreamWaitEvent(fs, c->instWritten, 0));
    return VXPT_OK;
}

// the host side of a device-mode refresh, per edit exactly as in host mode: the instance rows (edit: x, y,
// z, old id, new id -- the kept set; null: the scan), the light mapping, the light-update state and its
// remap.  The device work is left to inst_flush: at once, or at the end of a vxpt_set_blocks batch
int refresh_instances_device(vxpt_ctx *c, bool lights, bool full, const int *edit) {
    if (edit) edit_instance_set(c, edit[0], edit[1], edit[2], edit[3], edit[4]);
    else collect_instances(c);
    if (lights) {
        if (full) c->lightState.incremental = false;
        const unsigned prevN = c->nLights;
        std::vector<float> tri;
        std::vector<int> cells;
        std::vector<LightRun> runs;
        light_layout(c, false, tri, cells, runs);
        c->hRemap = light_id_map(c->lightState, c->lightMap, prevN, c->nLights);
        c->prevNumLights = prevN;
        c->lightsDirty = 1;
        c->instLightsDirty = true;
    }
    c->instDirty = true;
    return c->instBatch ? VXPT_OK : inst_flush(c);
}

// lights: rebuild the light table as a light update (full: scene init / reload; otherwise of the
// type the edits made it), or keep it (an edit of no emissive block, VoxelEngine.cu:1206, 1278)
int refresh_instances(vxpt_ctx *c, bool lights, bool full) { return refresh_instances_edit(c, lights, full, nullptr); }

int refresh_instances_edit(vxpt_ctx *c, bool lights, bool full, const int *edit) {
    if (!c->modelsLoaded) return VXPT_OK;
    if (c->instBuild == VXPT_INSTANCE_BUILD_DEVICE) return refresh_instances_device(c, lights, full, edit);
    ++c->ibStats[0];
    collect_instances(c);
    if (int r = build_tlas(c)) return r;
    if (lights) {
        if (full) c->lightState.incremental = false;
        const unsigned prevN = c->nLights;
        ++c->ibStats[2];
        if (int r = build_lights(c)) return r;
        if (int r = light_update(c, prevN)) return r;
    }
    const size_t n = c->instances.size() / 5;
    if (n == 0) return VXPT_OK;
    std::vector<int4> rows;
    std::vector<int> rowLight;
    instance_rows(c, rows, rowLight);
    if (int r = upload_vec(c, c->meshRow, rows.data(), rows.size())) return r;
    return upload_vec(c, c->meshRowLight, rowLight.data(), rowLight.size());
}

// closest instanced-mesh hit of n rays (8 floats each: o, tmin, d, tmax): out 4 floats (t, u, v,
// hit), ids 2 ints (instance row, triangle)
int vxpt_mesh_probe(vxpt_ctx *c, const float *rays, int n, int cull, float *out, int32_t *ids) {
    if (!c || !rays || !out || !ids || n < 0) return VXPT_ERR_ARG;
    if (n == 0) return VXPT_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    if (c->hRoot.empty()) c->hRoot.assign(kBlockTypes, make_int2(-1, -1));
    if (!c->blasRoot.p)
        if (int r = upload_vec(c, c->blasRoot, c->hRoot.data(), c->hRoot.size())) return r;
    // the probe's scratch grows with the largest call and lives with the context
    if (int r = upload_vec(c, c->probeRays, rays, (size_t)n * 8)) return r;
    if (grow(c, c->probeOut, (size_t)n * 4) || grow(c, c->probeIds, (size_t)n * 2)) return VXPT_ERR_HIP;
    HIPCHK(c, launch_mesh_probe(mesh_dev(c), c->probeRays.p, n, cull, c->probeOut.p, c->probeIds.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->probeOut.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ids, c->probeIds.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

// visibility rays against the instanced meshes: occluded[i] = 1 iff any triangle, either face,
// lies in [tmin, tmax] of ray i (8 floats: o, tmin, d, tmax)
int vxpt_mesh_occluded(vxpt_ctx *c, const float *rays, int n, uint8_t *occluded) {
    if (!c || !rays || !occluded || n < 0) return VXPT_ERR_ARG;
    if (n == 0) return VXPT_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    if (c->hRoot.empty()) c->hRoot.assign(kBlockTypes, make_int2(-1, -1));
    if (!c->blasRoot.p)
        if (int r = upload_vec(c, c->blasRoot, c->hRoot.data(), c->hRoot.size())) return r;
    if (int r = upload_vec(c, c->probeRays, rays, (size_t)n * 8)) return r;
    if (grow(c, c->probeOcc, (size_t)n)) return VXPT_ERR_HIP;
    HIPCHK(c, launch_mesh_occluded(mesh_dev(c), c->probeRays.p, n, c->probeOcc.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(occluded, c->probeOcc.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VXPT_OK;
}

// blocks.yaml (ids 13..29) + models.yaml + materials.yaml emission, then the OBJ meshes
int vxpt_load_models(vxpt_ctx *c, const char *root, int *loaded) {
    if (!c) return VXPT_ERR_ARG;
    const std::string dir = root ? root : c->dataDir;
    std::string line;
    std::map<std::string, std::string> modelFile;
    {
        std::ifstream f(c->dataDir + "/assets/models.yaml");
        if (!f) return fail(c, VXPT_ERR_IO, "missing assets/models.yaml");
        while (std::getline(f, line)) {
            const std::string tl = trim(line);
            if (tl.rfind("- {", 0) != 0) continue;
            auto m = parse_flow_map(tl);
            modelFile[m["id"]] = m["file"];
        }
    }
    std::map<std::string, std::map<std::string, std::string>> matProps;
    std::map<std::string, int> matIndex;  // MaterialParameter.materialId: the material's index in materials.yaml
    {
        std::ifstream f(c->dataDir + "/assets/materials.yaml");
        if (!f) return fail(c, VXPT_ERR_IO, "missing assets/materials.yaml");
        std::string cur;
        while (std::getline(f, line)) {
            const std::string tl = trim(line);
            if (tl.rfind("- id:", 0) == 0) {
                cur = trim(tl.substr(5));
                const int k = (int)matIndex.size();
                matIndex.emplace(cur, k);
            } else if (tl.rfind("properties:", 0) == 0) {
                matProps[cur] = parse_flow_map(tl);
            }
        }
    }
    std::ifstream fb(c->dataDir + "/assets/blocks.yaml");
    if (!fb) return fail(c, VXPT_ERR_IO, "missing assets/blocks.yaml");
    for (auto &b : c->blocks) b = vxpt_ctx::BlockDef{};
    int nLoaded = 0;
    while (std::getline(fb, line)) {
        const std::string tl = trim(line);
        if (tl.rfind("- {", 0) != 0) continue;
        auto m = parse_flow_map(tl);
        const int bid = std::atoi(m["id"].c_str());
        if (bid < 1 || bid >= kBlockTypes) continue;
        auto &bd = c->blocks[bid];
        bd.instanced = as_bool(m["instanced"]);
        bd.baseLight = as_bool(m["base_light"]);
        bd.lightBase = m.count("light_base") ? std::atoi(m["light_base"].c_str()) : 0;
        bd.model = m.count("model") ? m["model"] : "";
        // BlockManager::isEmissive: the block's flag or its material's; radiance from the material
        auto &mp = matProps[m["material"]];
        bd.emissive = as_bool(m["emissive"]) || as_bool(mp["is_emissive"]);
        if (as_bool(mp["is_emissive"]) && mp.count("emissive_radiance")) {
            const auto v = parse_list(mp["emissive_radiance"]);
            if (v.size() == 3) std::copy(v.begin(), v.end(), bd.emission);
        }
        if (bd.instanced) {
            // MaterialManager::createMaterialParameter (MaterialManager.cpp:150-190) for the mesh's
            // shading: an emissive material's albedo is its radiance (no textures on mesh materials here)
            MatDev md{{1.f, 1.f, 1.f}, 0.5f, 0.0f, 0, matIndex.count(m["material"]) ? matIndex[m["material"]] : 0, 0};
            if (mp.count("albedo")) {
                const auto v = parse_list(mp["albedo"]);
                if (v.size() == 3) std::copy(v.begin(), v.end(), md.albedo);
            }
            if (mp.count("roughness")) md.roughness = (float)std::atof(mp["roughness"].c_str());
            if (mp.count("metallic")) md.metallic = std::atof(mp["metallic"].c_str()) != 0.0;
            if (mp.count("translucency")) md.translucency = (float)std::atof(mp["translucency"].c_str());
            if (mp.count("is_thinfilm")) md.thin = as_bool(mp["is_thinfilm"]);
            if (mp.count("uv_scale")) md.uvScale = (float)std::atof(mp["uv_scale"].c_str());
            if (mp.count("use_world_grid_uv")) md.worldGridUV = as_bool(mp["use_world_grid_uv"]) ? 1 : 0;
            md.emissive = as_bool(mp["is_emissive"]) ? 1 : 0;
            if (md.emissive) std::copy(bd.emission, bd.emission + 3, md.albedo);
            c->mats[bid] = md;
        }
        if (!bd.instanced || bd.model.empty() || !modelFile.count(bd.model)) continue;
        if (load_obj(dir + "/" + modelFile[bd.model], bd.pos, bd.uv)) {
            bd.triangles = (int)(bd.pos.size() / 9);
            bd.pos.resize((size_t)bd.triangles * 9);
            bd.uv.resize((size_t)bd.triangles * 6);
            if (bd.triangles > 0) ++nLoaded;
        }
    }
    c->modelsLoaded = true;
    if (loaded) *loaded = nLoaded;
    // the farthest any loaded mesh reaches outside its unit cell (its instance is the cell's
    // translation): banded frames bound the primary hits' distance with it (nearest_surface)
    c->meshGrow = 1.0f;
    for (int b = 0; b < kBlockTypes; ++b)
        for (float v : c->blocks[b].pos) c->meshGrow = std::max(c->meshGrow, std::max(-v, v - 1.0f));
    ++c->worldVersion;  // a cached nearest-surface search used the old growth
    HIPCHK(c, hipSetDevice(c->dev));
    if (int r = build_blas(c)) return r;
    return refresh_instances(c, true, true);
}

int vxpt_get_model(vxpt_ctx *c, int block_id, float *pos, float *uv, int cap_triangles, int *n_triangles) {
    if (!c || block_id < 0 || block_id >= kBlockTypes) return VXPT_ERR_ARG;
    const auto &bd = c->blocks[block_id];
    if (n_triangles) *n_triangles = bd.triangles;
    const int n = std::min(cap_triangles, bd.triangles);
    if (pos && n > 0) std::copy(bd.pos.begin(), bd.pos.begin() + (size_t)n * 9, pos);
    if (uv && n > 0) std::copy(bd.uv.begin(), bd.uv.begin() + (size_t)n * 6, uv);
    return VXPT_OK;
}

int vxpt_get_instances(vxpt_ctx *c, int32_t *out, int cap, int *n_instances) {
    if (!c) return VXPT_ERR_ARG;
    const int n = (int)(c->instances.size() / 5);
    if (n_instances) *n_instances = n;
    if (out) std::copy(c->instances.begin(), c->instances.begin() + (size_t)std::min(cap, n) * 5, out);
    return VXPT_OK;
}

int vxpt_get_light_remap(vxpt_ctx *c, int32_t *remap, int cap, int *prev_num_lights, int *pending) {
    if (!c || cap < 0) return VXPT_ERR_ARG;
    if (prev_num_lights) *prev_num_lights = (int)c->prevNumLights;
    if (pending) *pending = c->lightsDirty;
    const int n = std::min(cap, (int)c->prevNumLights);
    if (remap && n > 0) {
        HIPCHK(c, hipSetDevice(c->dev));
        HIPCHK(c, hipMemcpyAsync(remap, c->lightRemap.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VXPT_OK;
}

int vxpt_get_lights(vxpt_ctx *c, uint32_t *mapping, int cap, int *n_mapped, uint32_t *n_lights, float *local_luminance) {
    if (!c) return VXPT_ERR_ARG;
    const int n = (int)(c->lightMap.size() / 3);
    if (n_mapped) *n_mapped = n;
    if (mapping) std::copy(c->lightMap.begin(), c->lightMap.begin() + (size_t)std::min(cap, n) * 3, mapping);
    if (n_lights) *n_lights = c->nLights;
    if (local_luminance) {
        if (c->lightLumOnDevice && c->nLights) {  // the device table's sum, fetched on demand
            AliasHead head{};
            HIPCHK(c, hipSetDevice(c->dev));
            HIPCHK(c, hipMemcpyAsync(&head, c->lightHead, sizeof(head), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->localLightLum = head.fsum;
            c->lightLumOnDevice = false;
        }
        *local_luminance = c->localLightLum;
    }
    return VXPT_OK;
}

}  // extern "C"

namespace vx::host {

// the instance / light side of one edit (old id -> block_id at a valid cell), after the grid changed
int edit_instances(vxpt_ctx *c, int x, int y, int z, int old, int block_id) {
    // the instance set only changes with an instanced block
    const auto inst = [&](int id) { return id > 0 && id < kBlockTypes && c->blocks[id].instanced; };
    if (!inst(old) && !inst(block_id)) return VXPT_OK;
    // deleteInstancedBlock / addInstancedBlock of an emissive block (VoxelEngine.cu:1206-1212,
    // 1278-1284): an incremental light update with the light instance removed / changed.  A light
    // base alone also carries its light's instance here (the instance set is always the grid's,
    // collectInstanceTransforms), so its edit counts as that light's.
    const auto light_obj = [&](int id) {
        if (!inst(id) || !c->modelsLoaded) return -1;
        if (c->blocks[id].emissive) return id - 1;
        for (int l = 1; l < kBlockTypes; ++l)
            if (c->blocks[l].instanced && c->blocks[l].emissive && c->blocks[l].lightBase == id) return l - 1;
        return -1;
    };
    const int lo = old != block_id ? light_obj(old) : -1, ln = old != block_id ? light_obj(block_id) : -1;
    if (lo >= 0) c->lightState.removed.insert(instance_id(c, lo, x, y, z));
    if (ln >= 0) c->lightState.changed.insert(instance_id(c, ln, x, y, z));
    if (lo >= 0 || ln >= 0) c->lightState.incremental = true;
    const int edit[5] = {x, y, z, old, block_id};
    return refresh_instances_edit(c, lo >= 0 || ln >= 0, false, edit);
}

}  // namespace vx::host

extern "C" {

int vxpt_set_instance_build(vxpt_ctx *c, int mode) {
    if (!c || (mode != VXPT_INSTANCE_BUILD_HOST && mode != VXPT_INSTANCE_BUILD_DEVICE)) return VXPT_ERR_ARG;
    if (mode == c->instBuild) return VXPT_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    for (hipStream_t fs : c->frontStreams) HIPCHK(c, hipStreamSynchronize(fs));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->instBuild = mode;
    // a loaded scene's tables, rebuilt whole in the new mode (before vxpt_load_models: applied there)
    return refresh_instances(c, true, true);
}

int vxpt_instance_build_stats(vxpt_ctx *c, uint32_t out[4]) {
    if (!c || !out) return VXPT_ERR_ARG;
    std::copy(c->ibStats, c->ibStats + 4, out);
    return VXPT_OK;
}

int vxpt_instance_build_ms(vxpt_ctx *c, float *ms) {
    if (!c || !ms) return VXPT_ERR_ARG;
    if (!c->ibTimed) return fail(c, VXPT_ERR_STATE, "no device instance refresh yet");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipEventSynchronize(c->ibEv[1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->ibEv[0], c->ibEv[1]));
    return VXPT_OK;
}

int vxpt_mesh_instance_count(vxpt_ctx *c, int *n, int *n_nodes) {
    if (!c) return VXPT_ERR_ARG;
    if (n) *n = c->nMeshInst;
    if (n_nodes) *n_nodes = c->nTlasNodes;
    return VXPT_OK;
}

int vxpt_lbvh_host(const float *boxes, const uint64_t *keys, int n, void *nodes, int32_t *order) {
    return lbvh::build_host(boxes, keys, n, static_cast<BvhNode *>(nodes), order) ? VXPT_OK : VXPT_ERR_ARG;
}

uint64_t vxpt_lbvh_key(int x, int y, int z, int object) { return lbvh::instance_key(x, y, z, object); }

int vxpt_lbvh_world_fits(int cx, int cy, int cz) {
    return cx > 0 && cy > 0 && cz > 0 && cx <= 67108863 && cy <= 67108863 && cz <= 67108863 &&
           lbvh::world_fits(cx * 32, cy * 32, cz * 32) ? 1 : 0;
}

int vxpt_bvh_depth(const float *boxes, int n, int leaf_max, int *max_depth, int *n_nodes) {
    if (!boxes || n < 0 || leaf_max < 1 || !max_depth) return VXPT_ERR_ARG;
    std::vector<float> box(boxes, boxes + (size_t)n * 6);
    std::vector<BvhNode> nodes;
    std::vector<int> order;
    const bool ok = build_bvh(box, leaf_max, nodes, order, max_depth);
    if (n_nodes) *n_nodes = (int)nodes.size();
    return ok ? VXPT_OK : VXPT_ERR_STATE;
}

}  // extern "C"
