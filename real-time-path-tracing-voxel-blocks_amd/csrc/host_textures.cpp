// vxpt -- host runtime, textures: the RGBA8 mip chains, their BC7 / BC5 / BC4 storage from cache files, the host
// codec (bcn.cpp) or the device encoders (bcn_encode.hip), the tables' read-out and the sampler probe.
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "bcn.hpp"
#include "bcn_decode.hpp"
#include "host_ctx.hpp"

extern "C" {

namespace {

// TextureManager::initWithMaterialPaths + LoadTexturesFromPaths (TextureManager.cu:133-330):
// every texture the cube materials name, in sorted path order (= texture id); decoded, square
// power-of-two, expanded to RGBA8 (1 channel -> (v,0,0,1), 2 -> (v,a,0,1), 3 -> (r,g,b,1): the
// unorm reads of the BC4/BC5/BC7 formats), levels 0..log2(size)-2 by 2x2 box averages truncated
// to 8 bits (fillMipmapKernel, :82-117, and its CPU twin, :390-414).  Binds mats[].tex[].
// paths / channels (optional): each loaded texture's material path and PNG channel count.
void build_mip_chains(vxpt_ctx *c, const std::string &base, std::vector<uchar4> &texels, std::vector<TexInfo> &table,
                      std::vector<std::string> *texPaths, std::vector<int> *channels) {
    std::vector<std::string> paths;
    for (int b = 1; b <= 12; ++b)
        for (int k = 0; k < 4; ++k)
            if (!c->texPath[b][k].empty()) paths.push_back(c->texPath[b][k]);
    std::sort(paths.begin(), paths.end());
    paths.erase(std::unique(paths.begin(), paths.end()), paths.end());
    std::map<std::string, int> idOf;
    for (const std::string &pth : paths) {
        int w, h, ch;
        std::vector<uint8_t> px;
        if (!decode_png(base + "/" + pth, w, h, ch, px)) continue;  // the reference skips it too (:180-187)
        if (w != h || w < 4 || (w & (w - 1)) != 0) continue;
        int maxLod = 0;
        while ((4 << maxLod) < w) ++maxLod;  // log2(w) - 2
        if (maxLod >= kMaxTexLevels) continue;
        TexInfo ti{};
        ti.size = w;
        ti.maxLod = maxLod;
        ti.off[0] = (unsigned)texels.size();
        texels.resize(texels.size() + (size_t)w * w);
        uchar4 *l0 = texels.data() + ti.off[0];
        for (size_t i = 0; i < (size_t)w * w; ++i) {
            const uint8_t *q = px.data() + i * ch;
            l0[i] = ch == 1 ? make_uchar4(q[0], 0, 0, 255)
                  : ch == 2 ? make_uchar4(q[0], q[1], 0, 255)
                  : ch == 3 ? make_uchar4(q[0], q[1], q[2], 255) : make_uchar4(q[0], q[1], q[2], q[3]);
        }
        for (int l = 1; l <= maxLod; ++l) {
            const int S = w >> l, P = S * 2;
            ti.off[l] = (unsigned)texels.size();
            texels.resize(texels.size() + (size_t)S * S);
            const uchar4 *src = texels.data() + ti.off[l - 1];
            uchar4 *dst = texels.data() + ti.off[l];
            for (int y = 0; y < S; ++y)
                for (int x = 0; x < S; ++x) {
                    const uchar4 a = src[(2 * y) * P + 2 * x], b2 = src[(2 * y) * P + 2 * x + 1];
                    const uchar4 c2 = src[(2 * y + 1) * P + 2 * x], d = src[(2 * y + 1) * P + 2 * x + 1];
                    dst[y * S + x] = make_uchar4((a.x + b2.x + c2.x + d.x) >> 2, (a.y + b2.y + c2.y + d.y) >> 2,
                                                 (a.z + b2.z + c2.z + d.z) >> 2, (a.w + b2.w + c2.w + d.w) >> 2);
                }
        }
        idOf[pth] = (int)table.size();
        table.push_back(ti);
        if (texPaths) texPaths->push_back(pth);
        if (channels) channels->push_back(ch);
    }
    for (int b = 1; b <= 12; ++b)
        for (int k = 0; k < 4; ++k) {
            const auto it = idOf.find(c->texPath[b][k]);
            c->mats[b].tex[k] = it == idOf.end() ? -1 : it->second;
        }
}

}  // namespace

// The RGBA8 texture set (the default): build_mip_chains' texels as they are, sampled by texel_f.
// The reference's block-compressed storage of the same chains is vxpt_load_textures_bc.
int vxpt_load_textures(vxpt_ctx *c, const char *root, int *loaded) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    const std::string base = root ? root : c->dataDir;
    std::vector<uchar4> texels;
    std::vector<TexInfo> table;
    build_mip_chains(c, base, texels, table, nullptr, nullptr);
    c->hTex = table;
    c->nTexels = texels.size();
    c->hTexBc.clear();
    c->nTexBlockBytes = 0;
    c->texBcOn = false;
    if (!table.empty()) {
        if (int r = upload_vec(c, c->texels, texels.data(), texels.size())) return r;
        if (int r = upload_vec(c, c->texTable, table.data(), table.size())) return r;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->texEnabled = table.empty() ? 0 : 1;
    if (loaded) *loaded = (int)table.size();
    return VXPT_OK;
}

namespace {

// device buffers of one encode, freed when it ends (a texture load is rare: nothing is kept)
struct BcEncTemp {
    uint32_t *src = nullptr;
    BcEncJob *jobs = nullptr;
    ~BcEncTemp() {
        if (src) hipFree(src);
        if (jobs) hipFree(jobs);
    }
};

void push_level_jobs(std::vector<BcEncJob> &jobs, uint32_t src, int w, int h, uint32_t dst, int bpb) {
    for (int by = 0; by < h / 4; ++by)
        for (int bx = 0; bx < w / 4; ++bx)
            jobs.push_back(BcEncJob{src, (uint32_t)w, (uint16_t)bx, (uint16_t)by, dst + (uint32_t)((size_t)by * (w / 4) + bx) * bpb});
}

// The jobs of each format (BC4, BC5, BC7) encoded into out on the context stream, one launch per
// format, between the events vxpt_bc_encode_ms reads; nTexels RGBA8 texels are uploaded for them.
int device_encode(vxpt_ctx *c, const uint8_t *rgba, size_t nTexels, const std::vector<BcEncJob> jobs[3], int quality,
                  uint8_t *out) {
    BcEncTemp tmp;
    const size_t nJobs = jobs[0].size() + jobs[1].size() + jobs[2].size();
    if (nJobs == 0) return VXPT_OK;
    for (auto &e : c->bcEv)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipMalloc((void **)&tmp.src, nTexels * 4));
    HIPCHK(c, hipMalloc((void **)&tmp.jobs, nJobs * sizeof(BcEncJob)));
    HIPCHK(c, hipMemcpyAsync(tmp.src, rgba, nTexels * 4, hipMemcpyHostToDevice, c->stream));
    size_t at = 0;
    for (int f = 0; f < 3; ++f) {
        if (!jobs[f].empty())
            HIPCHK(c, hipMemcpyAsync(tmp.jobs + at, jobs[f].data(), jobs[f].size() * sizeof(BcEncJob), hipMemcpyHostToDevice, c->stream));
        at += jobs[f].size();
    }
    HIPCHK(c, hipEventRecord(c->bcEv[0], c->stream));
    const int formats[3] = {bcn::kBc4, bcn::kBc5, bcn::kBc7};
    at = 0;
    for (int f = 0; f < 3; ++f) {
        HIPCHK(c, launch_bc_encode(formats[f], tmp.src, tmp.jobs + at, (int)jobs[f].size(), quality, out, c->stream));
        at += jobs[f].size();
    }
    HIPCHK(c, hipEventRecord(c->bcEv[1], c->stream));
    c->bcTimed = true;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the temporaries are freed on return
    return VXPT_OK;
}

}  // namespace

// The same set with every level as BC7 / BC5 / BC4 blocks (TextureManager.cu:189-330): the format
// from the PNG's channel count (:193-210), each level's blocks from its cache file or the encoder
// (bcn.hpp level_blocks; :271-287), every chain padded to 16 bytes so that BC7 / BC5 levels start
// aligned (a BC4 level is a multiple of 8).  VXPT_TEX_EXPAND decodes the blocks back into the
// RGBA8 buffer (same offsets as vxpt_load_textures) and samples that.
// VXPT_TEX_ENCODE_SEARCH: the levels without a cache file are encoded at quality 1 by the device
// encoders, straight into the block buffer, and read back only for the cache files and the expansion.
int vxpt_load_textures_bc(vxpt_ctx *c, const char *root, const char *cache_dir, int flags, int *loaded,
                          int *levels_from_cache) {
    if (!c) return VXPT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->dev));
    const std::string base = root ? root : c->dataDir;
    std::vector<uchar4> texels;
    std::vector<TexInfo> table;
    std::vector<std::string> texPaths;
    std::vector<int> channels;
    build_mip_chains(c, base, texels, table, &texPaths, &channels);
    std::vector<uint8_t> blocks, level;
    std::vector<TexBcInfo> bcTable;
    int cached = 0;
    const bool expand = (flags & VXPT_TEX_EXPAND) != 0, search = (flags & VXPT_TEX_ENCODE_SEARCH) != 0;
    const bool writeCache = (flags & VXPT_TEX_WRITE_CACHE) != 0;
    const std::string cacheDir = cache_dir ? cache_dir : "";
    std::vector<BcEncJob> jobs[3];  // search: the uncached levels' blocks by format (BC4, BC5, BC7)
    struct Pending { size_t tex; int lod; };
    std::vector<Pending> pending;
    for (size_t i = 0; i < table.size(); ++i) {
        TexBcInfo bi{};
        bi.format = bcn::format_of_channels(channels[i]);
        for (int l = 0; l <= table[i].maxLod; ++l) {
            const int S = table[i].size >> l;
            uint8_t *rgba = reinterpret_cast<uint8_t *>(texels.data() + table[i].off[l]);
            bool hit;
            if (search) {
                hit = bcn::read_cache_level(bi.format, S, cacheDir, texPaths[i], l, level);
                if (!hit) std::fill(level.begin(), level.end(), (uint8_t)0);
            } else {
                hit = bcn::level_blocks(bi.format, rgba, S, cacheDir, texPaths[i], l, writeCache, level);
            }
            cached += hit ? 1 : 0;
            if (blocks.size() + level.size() > 0xfffffff0ull) return fail(c, VXPT_ERR_ARG, "texture blocks exceed 4 GiB");
            bi.off[l] = (unsigned)blocks.size();
            blocks.insert(blocks.end(), level.begin(), level.end());
            if (search && !hit) {
                push_level_jobs(jobs[bi.format == bcn::kBc4 ? 0 : bi.format == bcn::kBc5 ? 1 : 2], table[i].off[l], S, S,
                                bi.off[l], bcn::bytes_per_block(bi.format));
                pending.push_back(Pending{i, l});
            } else if (expand) {
                bcn::decode(bi.format, level.data(), S / 4, S / 4, rgba);
            }
        }
        blocks.resize((blocks.size() + 15) & ~(size_t)15);
        bcTable.push_back(bi);
    }
    c->hTex = table;
    c->nTexels = texels.size();
    c->hTexBc = bcTable;
    c->nTexBlockBytes = blocks.size();
    c->texBcOn = !expand && !table.empty();
    if (!table.empty()) {
        if (!pending.empty()) {
            // the cached levels' bytes go up with the buffer; the kernels fill in the rest in place
            if (int r = upload_vec(c, c->texBlocks, blocks.data(), blocks.size())) return r;
            if (int r = device_encode(c, reinterpret_cast<const uint8_t *>(texels.data()), texels.size(), jobs, 1, c->texBlocks.p))
                return r;
            if (expand || (writeCache && !cacheDir.empty())) {
                HIPCHK(c, hipMemcpy(blocks.data(), c->texBlocks.p, blocks.size(), hipMemcpyDeviceToHost));
                for (const Pending &pd : pending) {
                    const int S = table[pd.tex].size >> pd.lod, fmt = bcTable[pd.tex].format;
                    const uint8_t *lv = blocks.data() + bcTable[pd.tex].off[pd.lod];
                    if (writeCache)
                        bcn::write_cache_level(cacheDir, texPaths[pd.tex], pd.lod, lv, (size_t)S * S / 16 * bcn::bytes_per_block(fmt));
                    if (expand)
                        bcn::decode(fmt, lv, S / 4, S / 4, reinterpret_cast<uint8_t *>(texels.data() + table[pd.tex].off[pd.lod]));
                }
            }
        } else if (!expand) {
            if (int r = upload_vec(c, c->texBlocks, blocks.data(), blocks.size())) return r;
        }
        if (expand) {
            if (int r = upload_vec(c, c->texels, texels.data(), texels.size())) return r;
        } else {
            if (int r = upload_vec(c, c->texBcTable, bcTable.data(), bcTable.size())) return r;
        }
        if (int r = upload_vec(c, c->texTable, table.data(), table.size())) return r;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->texEnabled = table.empty() ? 0 : 1;
    if (loaded) *loaded = (int)table.size();
    if (levels_from_cache) *levels_from_cache = cached;
    return VXPT_OK;
}

int vxpt_bc_encode_device(vxpt_ctx *c, int format, const uint8_t *rgba, int w, int h, int quality, void *blocks_out) {
    if (!c || (format != bcn::kBc4 && format != bcn::kBc5 && format != bcn::kBc7) || !rgba || w <= 0 || h <= 0 || (w & 3) ||
        (h & 3) || w > 262144 || h > 262144 || (quality != 0 && quality != 1) || !blocks_out)
        return VXPT_ERR_ARG;
    const size_t bytes = (size_t)(w / 4) * (h / 4) * bcn::bytes_per_block(format);
    if ((size_t)w * h > 0x40000000ull) return fail(c, VXPT_ERR_ARG, "image exceeds 2^30 texels");
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<BcEncJob> jobs[3];
    push_level_jobs(jobs[format == bcn::kBc4 ? 0 : format == bcn::kBc5 ? 1 : 2], 0u, w, h, 0u, bcn::bytes_per_block(format));
    uint8_t *out = nullptr;
    HIPCHK(c, hipMalloc((void **)&out, bytes));
    int r = device_encode(c, rgba, (size_t)w * h, jobs, quality, out);
    if (r == VXPT_OK && hipMemcpy(blocks_out, out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        r = fail(c, VXPT_ERR_HIP, "reading the encoded blocks back");
    hipFree(out);
    return r;
}

int vxpt_bc_encode_ms(vxpt_ctx *c, float *ms) {
    if (!c || !ms) return VXPT_ERR_ARG;
    if (!c->bcTimed) return fail(c, VXPT_ERR_STATE, "no device encode yet");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipEventSynchronize(c->bcEv[1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->bcEv[0], c->bcEv[1]));
    return VXPT_OK;
}

int vxpt_enable_textures(vxpt_ctx *c, int on) {
    if (!c) return VXPT_ERR_ARG;
    c->texEnabled = (on && !c->hTex.empty()) ? 1 : 0;
    return VXPT_OK;
}

// the loaded table: per texture size, maxLod, then maxLod + 1 level offsets (in texels)
int vxpt_texture_table(vxpt_ctx *c, int32_t *out, int cap, int *n_textures, int64_t *n_texels) {
    if (!c) return VXPT_ERR_ARG;
    int k = 0;
    for (const TexInfo &t : c->hTex) {
        if (out && k + 2 + t.maxLod + 1 > cap) return VXPT_ERR_ARG;
        if (out) {
            out[k] = t.size;
            out[k + 1] = t.maxLod;
            for (int l = 0; l <= t.maxLod; ++l) out[k + 2 + l] = (int32_t)t.off[l];
        }
        k += 2 + t.maxLod + 1;
    }
    if (n_textures) *n_textures = (int)c->hTex.size();
    if (n_texels) *n_texels = (int64_t)c->nTexels;
    return VXPT_OK;
}

// the block table: per texture format, size, maxLod, then maxLod + 1 level offsets (in bytes)
int vxpt_texture_table_bc(vxpt_ctx *c, int64_t *out, int cap, int *n_textures, int64_t *n_bytes) {
    if (!c) return VXPT_ERR_ARG;
    int k = 0;
    for (size_t i = 0; i < c->hTexBc.size(); ++i) {
        const TexInfo &t = c->hTex[i];
        if (out && k + 3 + t.maxLod + 1 > cap) return VXPT_ERR_ARG;
        if (out) {
            out[k] = c->hTexBc[i].format;
            out[k + 1] = t.size;
            out[k + 2] = t.maxLod;
            for (int l = 0; l <= t.maxLod; ++l) out[k + 3 + l] = (int64_t)c->hTexBc[i].off[l];
        }
        k += 3 + t.maxLod + 1;
    }
    if (n_textures) *n_textures = (int)c->hTexBc.size();
    if (n_bytes) *n_bytes = (int64_t)c->nTexBlockBytes;
    return VXPT_OK;
}

}  // extern "C"

extern "C" int vxpt_probe_texture(vxpt_ctx *c, int tex_id, int n, const float *uvlod, float *out) {
    if (!c || n <= 0 || !uvlod || !out) return VXPT_ERR_ARG;
    if (tex_id < 0 || tex_id >= (int)c->hTex.size()) return fail(c, VXPT_ERR_ARG, "no such texture");
    HIPCHK(c, hipSetDevice(c->dev));
    float *din;
    float4 *dout;
    HIPCHK(c, hipMalloc(&din, (size_t)n * 12));
    HIPCHK(c, hipMalloc(&dout, (size_t)n * 16));
    HIPCHK(c, hipMemcpyAsync(din, uvlod, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_probe_texture(c->texTable.p, c->texels.p, c->texBcOn ? c->texBcTable.p : nullptr,
                                   c->texBcOn ? c->texBlocks.p : nullptr, tex_id, n, din, dout, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(din);
    hipFree(dout);
    return VXPT_OK;
}
