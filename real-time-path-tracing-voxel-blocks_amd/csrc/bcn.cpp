// Block-compressed textures, host side (bcn.hpp): decode, encoder, cache files, and their C entry
// points (include/vxpt.h).  Nothing here touches the GPU.
#include "bcn.hpp"

#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>

#include "../../include/vxpt.h"
#include "bcn_decode.hpp"

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

namespace {

// 16 values -> one BC4 channel block: endpoints max, min in the 8-value mode (e0 > e1), nearest
// palette entry per texel (ties: the lower index); a constant block is e0 = e1 with index 0
void encode_bc4(const int v[16], uint8_t out[8]) {
    int mx = v[0], mn = v[0];
    for (int t = 1; t < 16; ++t) {
        mx = v[t] > mx ? v[t] : mx;
        mn = v[t] < mn ? v[t] : mn;
    }
    uint64_t bitsOut = (uint64_t)mx | ((uint64_t)mn << 8);
    if (mx > mn) {
        int pal[8] = {mx, mn};
        for (int k = 1; k <= 6; ++k) pal[k + 1] = ((7 - k) * mx + k * mn) / 7;
        for (int t = 0; t < 16; ++t) {
            int best = 0, bestErr = 1 << 30;
            for (int i = 0; i < 8; ++i) {
                const int e = v[t] > pal[i] ? v[t] - pal[i] : pal[i] - v[t];
                if (e < bestErr) {
                    bestErr = e;
                    best = i;
                }
            }
            bitsOut |= (uint64_t)best << (16 + 3 * t);
        }
    }
    for (int i = 0; i < 8; ++i) out[i] = (uint8_t)(bitsOut >> (8 * i));
}

struct Bits128 {
    uint64_t lo = 0, hi = 0;
    int pos = 0;
    void put(uint32_t v, int n) {
        for (int i = 0; i < n; ++i, ++pos)
            if ((v >> i) & 1u) (pos < 64 ? lo : hi) |= 1ull << (pos & 63);
    }
};

// a mode-6 endpoint is 8 bits per channel whose low bit is the endpoint's one p-bit: the value
// with low bit p nearest to num / den (ties: the lower)
int nearest_with_lsb(int num, int den, int p) {
    int best = p, bestErr = 1 << 30;
    const int x = num / den, first = x < 4 ? p : (((x - 3) & ~1) | p);
    for (int e = first; e < 256 && e <= x + 3; e += 2) {
        const int d = e * den - num, err = d < 0 ? -d : d;
        if (err < bestErr) {
            bestErr = err;
            best = e;
        }
    }
    return best;
}
// the p-bit (0 on a tie) and channel values for targets num[c] / den that leave the smaller summed distance
void quantise_endpoint(const int num[4], int den, int e[4]) {
    int bestSum = 1 << 30;
    for (int p = 0; p < 2; ++p) {
        int q[4], sum = 0;
        for (int c = 0; c < 4; ++c) {
            q[c] = nearest_with_lsb(num[c], den, p);
            const int d = q[c] * den - num[c];
            sum += d < 0 ? -d : d;
        }
        if (sum < bestSum) {
            bestSum = sum;
            for (int c = 0; c < 4; ++c) e[c] = q[c];
        }
    }
}
// indices of the 16 texels on the palette of e0, e1 (nearest in summed squared error, ties: the lower
// index); returns the block's largest absolute channel error
int fit_indices(const int px[16][4], const int e0[4], const int e1[4], int idx[16]) {
    int pal[16][4];
    for (int i = 0; i < 16; ++i)
        for (int c = 0; c < 4; ++c) pal[i][c] = lerp64(e0[c], e1[c], kBc7Weight[12 + i]);
    int worst = 0;
    for (int t = 0; t < 16; ++t) {
        int best = 0, bestErr = 1 << 30;
        for (int i = 0; i < 16; ++i) {
            int err = 0;
            for (int c = 0; c < 4; ++c) err += (px[t][c] - pal[i][c]) * (px[t][c] - pal[i][c]);
            if (err < bestErr) {
                bestErr = err;
                best = i;
            }
        }
        idx[t] = best;
        for (int c = 0; c < 4; ++c) {
            const int d = px[t][c] - pal[best][c];
            worst = (d < 0 ? -d : d) > worst ? (d < 0 ? -d : d) : worst;
        }
    }
    return worst;
}

// 16 RGBA texels -> a BC7 mode-6 block.  Endpoints: the corners of the block's colour box along its
// diagonal, each channel's direction taken from the sign of its covariance with the widest channel;
// kept unless the block's mean colour as both endpoints has the smaller largest error.
void encode_bc7(const int px[16][4], uint8_t out[16]) {
    int mn[4], mx[4], sum[4];
    for (int c = 0; c < 4; ++c) {
        mn[c] = mx[c] = sum[c] = px[0][c];
        for (int t = 1; t < 16; ++t) {
            mn[c] = px[t][c] < mn[c] ? px[t][c] : mn[c];
            mx[c] = px[t][c] > mx[c] ? px[t][c] : mx[c];
            sum[c] += px[t][c];
        }
    }
    int ref = 0;
    for (int c = 1; c < 4; ++c)
        if (mx[c] - mn[c] > mx[ref] - mn[ref]) ref = c;
    int lo[4], hi[4];
    for (int c = 0; c < 4; ++c) {
        long long cov = 0;  // 256 x the covariance with the widest channel
        for (int t = 0; t < 16; ++t) cov += (long long)(16 * px[t][c] - sum[c]) * (16 * px[t][ref] - sum[ref]);
        lo[c] = cov < 0 ? mx[c] : mn[c];
        hi[c] = cov < 0 ? mn[c] : mx[c];
    }
    int e0[4], e1[4], idx[16];
    quantise_endpoint(lo, 1, e0);
    quantise_endpoint(hi, 1, e1);
    const int worst = fit_indices(px, e0, e1, idx);
    int m[4], midx[16];
    quantise_endpoint(sum, 16, m);
    if (fit_indices(px, m, m, midx) < worst) {
        for (int c = 0; c < 4; ++c) e0[c] = e1[c] = m[c];
        for (int t = 0; t < 16; ++t) idx[t] = midx[t];
    }
    if (idx[0] >= 8) {  // the anchor's index keeps its high bit 0: swap the endpoints
        for (int c = 0; c < 4; ++c) {
            const int s = e0[c];
            e0[c] = e1[c];
            e1[c] = s;
        }
        for (int t = 0; t < 16; ++t) idx[t] = 15 - idx[t];
    }
    Bits128 w;
    w.put(1u << 6, 7);
    for (int c = 0; c < 4; ++c) {
        w.put((uint32_t)e0[c] >> 1, 7);
        w.put((uint32_t)e1[c] >> 1, 7);
    }
    w.put((uint32_t)e0[0] & 1u, 1);
    w.put((uint32_t)e1[0] & 1u, 1);
    w.put((uint32_t)idx[0], 3);
    for (int t = 1; t < 16; ++t) w.put((uint32_t)idx[t], 4);
    for (int i = 0; i < 8; ++i) {
        out[i] = (uint8_t)(w.lo >> (8 * i));
        out[8 + i] = (uint8_t)(w.hi >> (8 * i));
    }
}

}  // namespace

void encode(int format, const uint8_t *rgba, int w, int h, uint8_t *blocks) {
    const int nbx = w / 4, nby = h / 4, bpb = bytes_per_block(format);
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            int px[16][4];
            for (int t = 0; t < 16; ++t)
                for (int c = 0; c < 4; ++c) px[t][c] = rgba[(((size_t)by * 4 + (t >> 2)) * w + (size_t)bx * 4 + (t & 3)) * 4 + c];
            uint8_t *o = blocks + ((size_t)by * nbx + bx) * bpb;
            if (format == kBc7) {
                encode_bc7(px, o);
            } else {
                int v[16];
                for (int ch = 0; ch < (format == kBc5 ? 2 : 1); ++ch) {
                    for (int t = 0; t < 16; ++t) v[t] = px[t][ch];
                    encode_bc4(v, o + 8 * ch);
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

bool level_blocks(int format, const uint8_t *rgba, int size, const std::string &cacheDir, const std::string &texPath,
                  int lod, bool writeCache, std::vector<uint8_t> &out) {
    const size_t bytes = (size_t)size * size / 16 * bytes_per_block(format);
    out.resize(bytes);
    const std::string file = cacheDir.empty() ? std::string() : cache_path(cacheDir, texPath, lod);
    if (!file.empty()) {
        std::error_code ec;
        const auto fsz = std::filesystem::file_size(file, ec);
        if (!ec && fsz == bytes) {
            std::ifstream f(file, std::ios::binary);
            if (f.read(reinterpret_cast<char *>(out.data()), (std::streamsize)bytes)) return true;
        }
    }
    encode(format, rgba, size, size, out.data());
    if (!file.empty() && writeCache) {
        std::error_code ec;
        std::filesystem::create_directories(std::filesystem::path(file).parent_path(), ec);
        std::ofstream f(file, std::ios::binary | std::ios::trunc);
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)bytes);
    }
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
