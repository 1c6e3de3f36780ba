// Host side of the block-compressed textures: whole-image decode (over bcn_decode.hpp, the body the
// sampler runs), the deterministic encoder, and the reference's texture-cache files.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace vx {
namespace bcn {

// format from a PNG's channel count (TextureManager.cu:193-210): 1 -> BC4, 2 -> BC5, 3 / 4 -> BC7
int format_of_channels(int ch);
// blocks: nbx x nby blocks, rows top-down -> rgba: 4 nby rows of 4 nbx RGBA8 texels
void decode(int format, const uint8_t *blocks, int nbx, int nby, uint8_t *rgba);
// rgba: h rows of w RGBA8 texels (w, h multiples of 4) -> (w / 4) x (h / 4) blocks.  BC4 encodes
// .x, BC5 .x and .y.  Integer arithmetic only: the same bytes on every run and machine.  quality 0:
// the fast encoder, 1: the search (bcn_encode.hpp, the bodies the device encoders run)
void encode(int format, const uint8_t *rgba, int w, int h, uint8_t *blocks, int quality = 0);
// <cache_dir>/<name>_lod_<lod>.bin, <name> as TextureManager.cu:168-173 derives it from the path
// the material names: what follows the first '/', up to ".png"
std::string cache_path(const std::string &cacheDir, const std::string &texPath, int lod);
// The two halves of level_blocks' cache rule: out = the cache file's bytes (true) when cacheDir is
// non-empty and the file holds exactly size^2 / 16 blocks, else out is only sized (false); and the
// write of an encoded level (nothing when cacheDir is empty)
bool read_cache_level(int format, int size, const std::string &cacheDir, const std::string &texPath, int lod,
                      std::vector<uint8_t> &out);
void write_cache_level(const std::string &cacheDir, const std::string &texPath, int lod, const uint8_t *blocks, size_t bytes);
// One size x size level as blocks: the cache file's bytes if cacheDir is non-empty and the file
// holds exactly size^2 / 16 blocks (a file of another size is ignored); else the encoded level,
// written to the cache when writeCache.  Returns true when the bytes came from the cache.
bool level_blocks(int format, const uint8_t *rgba, int size, const std::string &cacheDir, const std::string &texPath,
                  int lod, bool writeCache, std::vector<uint8_t> &out);

}  // namespace bcn
}  // namespace vx
