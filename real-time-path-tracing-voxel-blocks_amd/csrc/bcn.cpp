// Block-compressed textures, host side (bcn.hpp): decode, encoder, cache files, and their C entry
// points (include/vxpt.h).  Nothing here touches the GPU.
#include "bcn.hpp"

#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>

#include "../../include/vxpt.h"
#include "bcn_decode.hpp"
#include "bcn_encode.hpp"

namespace vx {
namespace bcn {

int format_of_channels(int ch) { return ch == 1 ? kBc4 : ch == 2 ? kBc5 : kBc7; }

void decode(int format, const uint8_t *blocks, int nbx, int nby, uint8_t *rgba) {
    const int bpb = bytes_per_block(format), W = 4 * nbx;
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            Block128 b{};
            std::memcpy(b.w, blocks + ((size_t)by * nbx + bx) * bpb, bpb);
            for (int t = 0; t < 16; ++t) {
                const Rgba c = texel(format, b, t);
                uint8_t *o = rgba + (((size_t)by * 4 + (t >> 2)) * W + (size_t)bx * 4 + (t & 3)) * 4;
                o[0] = (uint8_t)c.r;
                o[1] = (uint8_t)c.g;
                o[2] = (uint8_t)c.b;
                o[3] = (uint8_t)c.a;
            }
        }
}

void encode(int format, const uint8_t *rgba, int w, int h, uint8_t *blocks, int quality) {
    const int nbx = w / 4, nby = h / 4, bpb = bytes_per_block(format);
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            uint32_t px[16];
            for (int y = 0; y < 4; ++y) std::memcpy(px + 4 * y, rgba + (((size_t)by * 4 + y) * w + (size_t)bx * 4) * 4, 16);
            uint8_t *o = blocks + ((size_t)by * nbx + bx) * bpb;
            if (format == kBc7) {
                uint32_t out[4];
                enc::encode_bc7_host(px, quality, out);
                std::memcpy(o, out, 16);
            } else {
                for (int ch = 0; ch < (format == kBc5 ? 2 : 1); ++ch) {
                    const uint64_t bitsOut = enc::encode_bc4(px, ch, quality);
                    std::memcpy(o + 8 * ch, &bitsOut, 8);
                }
            }
        }
}

std::string cache_path(const std::string &cacheDir, const std::string &texPath, int lod) {
    const size_t start = texPath.find('/') + 1;  // npos + 1 = 0: no directory part
    const size_t end = texPath.find(".png");
    const std::string name = texPath.substr(start, end == std::string::npos ? end : end - start);
    return (std::filesystem::path(cacheDir) / name).string() + "_lod_" + std::to_string(lod) + ".bin";
}

bool read_cache_level(int format, int size, const std::string &cacheDir, const std::string &texPath, int lod,
                      std::vector<uint8_t> &out) {
    const size_t bytes = (size_t)size * size / 16 * bytes_per_block(format);
    out.resize(bytes);
    if (cacheDir.empty()) return false;
    const std::string file = cache_path(cacheDir, texPath, lod);
    std::error_code ec;
    const auto fsz = std::filesystem::file_size(file, ec);
    if (ec || fsz != bytes) return false;
    std::ifstream f(file, std::ios::binary);
    return (bool)f.read(reinterpret_cast<char *>(out.data()), (std::streamsize)bytes);
}

void write_cache_level(const std::string &cacheDir, const std::string &texPath, int lod, const uint8_t *blocks, size_t bytes) {
    if (cacheDir.empty()) return;
    const std::string file = cache_path(cacheDir, texPath, lod);
    std::error_code ec;
    std::filesystem::create_directories(std::filesystem::path(file).parent_path(), ec);
    std::ofstream f(file, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char *>(blocks), (std::streamsize)bytes);
}

bool level_blocks(int format, const uint8_t *rgba, int size, const std::string &cacheDir, const std::string &texPath,
                  int lod, bool writeCache, std::vector<uint8_t> &out) {
    if (read_cache_level(format, size, cacheDir, texPath, lod, out)) return true;
    encode(format, rgba, size, size, out.data());
    if (writeCache) write_cache_level(cacheDir, texPath, lod, out.data(), out.size());
    return false;
}

}  // namespace bcn
}  // namespace vx

using namespace vx;

static bool bc_format_ok(int f) { return f == bcn::kBc4 || f == bcn::kBc5 || f == bcn::kBc7; }

extern "C" int vxpt_bc_decode(int format, const void *blocks, int n_blocks_x, int n_blocks_y, uint8_t *rgba_out) {
    if (!bc_format_ok(format) || !blocks || n_blocks_x <= 0 || n_blocks_y <= 0 || !rgba_out) return VXPT_ERR_ARG;
    bcn::decode(format, static_cast<const uint8_t *>(blocks), n_blocks_x, n_blocks_y, rgba_out);
    return VXPT_OK;
}

extern "C" int vxpt_bc_encode(int format, const uint8_t *rgba, int w, int h, void *blocks_out) {
    if (!bc_format_ok(format) || !rgba || w <= 0 || h <= 0 || (w & 3) || (h & 3) || !blocks_out) return VXPT_ERR_ARG;
    bcn::encode(format, rgba, w, h, static_cast<uint8_t *>(blocks_out));
    return VXPT_OK;
}

extern "C" int vxpt_bc_encode_q(int format, const uint8_t *rgba, int w, int h, int quality, void *blocks_out) {
    if (!bc_format_ok(format) || !rgba || w <= 0 || h <= 0 || (w & 3) || (h & 3) || (quality != 0 && quality != 1) || !blocks_out)
        return VXPT_ERR_ARG;
    bcn::encode(format, rgba, w, h, static_cast<uint8_t *>(blocks_out), quality);
    return VXPT_OK;
}

extern "C" int vxpt_bc_cache_path(const char *cache_dir, const char *tex_path, int lod, char *out, int cap) {
    if (!cache_dir || !tex_path || lod < 0 || !out || cap <= 0) return VXPT_ERR_ARG;
    const std::string p = bcn::cache_path(cache_dir, tex_path, lod);
    if ((int)p.size() + 1 > cap) return VXPT_ERR_ARG;
    std::memcpy(out, p.c_str(), p.size() + 1);
    return VXPT_OK;
}

extern "C" int vxpt_bc_level(int format, const uint8_t *rgba, int size, const char *cache_dir, const char *tex_path,
                             int lod, int flags, void *blocks_out, int *from_cache) {
    if (!bc_format_ok(format) || !rgba || size < 4 || (size & (size - 1)) || !tex_path || lod < 0 || !blocks_out)
        return VXPT_ERR_ARG;
    std::vector<uint8_t> out;
    const bool hit = bcn::level_blocks(format, rgba, size, cache_dir ? cache_dir : "", tex_path, lod,
                                       (flags & VXPT_TEX_WRITE_CACHE) != 0, out);
    std::memcpy(blocks_out, out.data(), out.size());
    if (from_cache) *from_cache = hit ? 1 : 0;
    return VXPT_OK;
}
