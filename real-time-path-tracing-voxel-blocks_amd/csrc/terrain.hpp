// vxpt -- the terrain generator's per-column and per-cell bodies (VoxelSceneGen.cu:341-388), shared by
// the host generator (vxpt_generate_terrain, vxpt_terrain_host) and the kernels (terrain.hip).
// No HIP is needed to include it.
//
// Everything is float32 in the reference's operation order: the library is built with
// -ffp-contract=off, the one fused operation is the explicit fmaf of the column height, and no
// division happens here (the caller passes freq = 1 / freq_den).  Host and device therefore produce
// the same bits.  The noise reads a 256-byte permutation table through a plain pointer: a context
// member on the host, a copy in LDS on the device.
#pragma once
#include <cmath>
#include <cstdint>
#include <random>
#include <utility>

#if defined(__HIPCC__)
#define TER_HD __host__ __device__
#else
#define TER_HD
#endif

namespace vx {
namespace ter {

// the window of one generated world: chunk counts, cells added to the window's x, y, z before the
// noise / height compare, and the generator's settings
struct Window {
    int cx, cy, cz;
    int ox, oy, oz;
    float freq, width;  // 1 / freq_den, height_scale
    int keepBalls, globalY;
};

// the permutation of siv::BasicPerlinNoise<float>(seed) (PerlinNoise.hpp:229-494): a Fisher-Yates
// shuffle driven by std::mt19937
inline void permutation(uint32_t seed, uint8_t p[256]) {
    for (int i = 0; i < 256; ++i) p[i] = (uint8_t)i;
    std::mt19937 g(seed);
    for (int i = 1; i < 256; ++i) {
        const uint64_t r = (uint64_t)g() % (uint64_t)(i + 1);
        std::swap(p[i], p[r]);
    }
}

TER_HD inline float fade(float t) { return t * t * t * (t * (t * 6 - 15) + 10); }
TER_HD inline float lerp(float a, float b, float t) { return a + (b - a) * t; }
TER_HD inline float grad(uint8_t hash, float x, float y, float z) {
    const uint8_t h = hash & 15;
    const float u = h < 8 ? x : y;
    const float v = h < 4 ? y : (h == 12 || h == 14 ? x : z);
    return ((h & 1) == 0 ? u : -u) + ((h & 2) == 0 ? v : -v);
}
TER_HD inline float noise(const uint8_t *p, float x, float y, float z) {
    const float X = floorf(x), Y = floorf(y), Z = floorf(z);
    const int ix = (int)X & 255, iy = (int)Y & 255, iz = (int)Z & 255;
    const float fx = x - X, fy = y - Y, fz = z - Z;
    const float u = fade(fx), v = fade(fy), w = fade(fz);
    const uint8_t A = (p[ix] + iy) & 255, B = (p[(ix + 1) & 255] + iy) & 255;
    const uint8_t AA = (p[A] + iz) & 255, AB = (p[(A + 1) & 255] + iz) & 255;
    const uint8_t BA = (p[B] + iz) & 255, BB = (p[(B + 1) & 255] + iz) & 255;
    const float q0 = lerp(grad(p[AA], fx, fy, fz), grad(p[BA], fx - 1, fy, fz), u);
    const float q1 = lerp(grad(p[AB], fx, fy - 1, fz), grad(p[BB], fx - 1, fy - 1, fz), u);
    const float q2 = lerp(grad(p[(AA + 1) & 255], fx, fy, fz - 1), grad(p[(BA + 1) & 255], fx - 1, fy, fz - 1), u);
    const float q3 = lerp(grad(p[(AB + 1) & 255], fx, fy - 1, fz - 1), grad(p[(BB + 1) & 255], fx - 1, fy - 1, fz - 1), u);
    return lerp(lerp(q0, q1, v), lerp(q2, q3, v), w);
}
TER_HD inline float octave01(const uint8_t *p, float x, float y, int oct) {
    float r = 0, a = 1;
    for (int i = 0; i < oct; ++i) {
        r += noise(p, x, y, (float)0.34567) * a;
        x *= 2;
        y *= 2;
        a *= 0.5f;
    }
    if (r <= -1.0f) return 0.0f;
    if (1.0f <= r) return 1.0f;
    return r * 0.5f + 0.5f;
}

// the height of the column at global cell (gx, gz), four octaves
TER_HD inline float column_height(const uint8_t *p, int gx, int gz, float freq, float width) {
    const float n = octave01(p, (float)gx * freq, (float)gz * freq, 4);
    float h = fmaf(n, 1.4f, -0.7f);  // nvcc --fmad=true contraction of n*1.4f-0.7f
    h = fmaxf(0.1f, (h + 0.25f) * width);
    return fminf(h, width * 0.9f);
}

// the id of the cell at compared height gy in a column of height h; ly is its row in its chunk and
// (gx, gz) its global column (the shader balls sit at row 7 of every chunk layer)
TER_HD inline uint8_t cell_id(float h, float width, int gy, int ly, int gx, int gz, bool keepBalls) {
    uint8_t id = 0;
    const float yy = (float)gy;
    if (yy < h) {
        const float d = h - yy;
        if (h < width * (0.25f + 0.05f)) id = d < 3.5f ? 1 : 7;
        else if (h < width * (0.25f + 0.6f) && h > width * (0.25f + 0.3f)) id = d < 5.5f ? 3 : 7;
        else id = d < 1.5f ? 2 : (d < 5.5f ? 3 : 7);
    }
    if (keepBalls && ly == 7 && gz == 43 && gx >= 30 && gx <= 39) {
        const int k = gx - 30;  // ids 17, 21, 22, ... 29 (no table: a kernel would index it in scratch)
        id = (uint8_t)(k == 0 ? 17 : 20 + k);
    }
    return id;
}

// chunk ch of the window: the global x / z of its first column and the height its row 0 compares
TER_HD inline void chunk_origin(const Window &w, int ch, int &gox, int &goy, int &goz) {
    gox = w.ox + (ch % w.cx) * 32;
    goz = w.oz + ((ch / w.cx) % w.cz) * 32;
    goy = w.oy + (w.globalY ? (ch / (w.cx * w.cz)) * 32 : 0);
}

// host generator: the chunk-major ids (x + 32 * (z + 32 * y) per 32^3 chunk; chunks x-major, then z,
// then y) of the window
inline void generate_host(const Window &w, const uint8_t *p, uint8_t *ids) {
    for (int ch = 0; ch < w.cx * w.cy * w.cz; ++ch) {
        int gox, goy, goz;
        chunk_origin(w, ch, gox, goy, goz);
        float hmap[32][32];
        for (int z = 0; z < 32; ++z)
            for (int x = 0; x < 32; ++x) hmap[z][x] = column_height(p, gox + x, goz + z, w.freq, w.width);
        for (int y = 0; y < 32; ++y)
            for (int z = 0; z < 32; ++z)
                for (int x = 0; x < 32; ++x)
                    ids[(size_t)ch * 32768 + x + 32 * (z + 32 * y)] =
                        cell_id(hmap[z][x], w.width, goy + y, y, gox + x, goz + z, w.keepBalls != 0);
    }
}

}  // namespace ter
}  // namespace vx
