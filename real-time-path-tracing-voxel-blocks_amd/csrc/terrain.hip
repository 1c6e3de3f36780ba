// vxpt -- the Perlin terrain generated on gfx950 (vxpt_generate_terrain_ex).  The
// host generator runs the same bodies (terrain.hpp), so the ids are the host's bit for bit; the
// kernels behind them (world.hip) build the tables, and k_terrain_mirrors adds the two per-brick /
// per-block counts the host mirrors hold beside what those tables already contain.
#include "terrain.hpp"
#include "vx_internal.hpp"
#include "world_build.hpp"

namespace vx {
namespace {

// One lane per (x, z) column of the window, four octaves of noise.  The 256-byte permutation table
// sits in LDS: the eight dependent look-ups per octave are byte reads at lane-varying addresses.
__global__ __launch_bounds__(256) void k_terrain_height(ter::Window t, const uint8_t *__restrict__ perm,
                                                         float *__restrict__ height) {
    __shared__ uint8_t p[256];
    p[threadIdx.x] = perm[threadIdx.x];
    __syncthreads();
    const int wx = t.cx * 32;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)wx * t.cz * 32) return;
    const int x = (int)(i % wx), z = (int)(i / wx);
    height[i] = ter::column_height(p, t.ox + x, t.oz + z, t.freq, t.width);
}

// One lane per 16 consecutive x cells of the chunk-major ids: a chunk row of 32 cells is two lanes,
// consecutive lanes store consecutive 16 bytes.  The lane's 16 heights are four aligned float4 loads
// (the window's width is a multiple of 32 columns); every y layer of chunks re-reads the same plane,
// which stays in L2.
__global__ __launch_bounds__(256) void k_terrain_fill(ter::Window t, const float *__restrict__ height,
                                                       uint8_t *__restrict__ ids) {
    const size_t nChunks = (size_t)t.cx * t.cy * t.cz;
    const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (lane >= nChunks * 2048) return;
    const int ch = (int)(lane >> 11), r = (int)(lane & 2047);
    const int x0 = (r & 1) * 16, z = (r >> 1) & 31, y = r >> 6;
    int gox, goy, goz;
    ter::chunk_origin(t, ch, gox, goy, goz);
    const int wx = t.cx * 32;
    // the column's place in the height plane is relative to the window, not to the origin
    const float4 *h4 = reinterpret_cast<const float4 *>(height + (size_t)(goz - t.oz + z) * wx + (gox - t.ox + x0));
    uint32_t out[4];
    for (int q = 0; q < 4; ++q) {
        const float4 h = h4[q];
        const float hs[4] = {h.x, h.y, h.z, h.w};
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + 4 * q + k;
            v |= (uint32_t)ter::cell_id(hs[k], t.width, goy + y, y, gox + x, goz + z, t.keepBalls != 0) << (8 * k);
        }
        out[q] = v;
    }
    reinterpret_cast<uint4 *>(ids)[lane] = make_uint4(out[0], out[1], out[2], out[3]);
}

// One wave64 per 16^3 macro cell, one lane per brick, as k_wb_occupancy: the brick's non-air cells
// counted from its 64 brick-major bytes, and the macro cell's cube cells (a wave sum of the masks'
// bit counts) added to its 64^3 block.  Integer sums: their order cannot change the result.
__global__ __launch_bounds__(64) void k_terrain_mirrors(WbWorld w, uint8_t *__restrict__ nonAir,
                                                         int *__restrict__ topCount) {
    const int MX = w.cx * 2, MZ = w.cz * 2;
    const size_t m = blockIdx.x;
    const int l = threadIdx.x;
    const size_t b = m * 64 + l;
    const uint4 *src = reinterpret_cast<const uint4 *>(w.bricks + b * 64);
    int n = 0;
    for (int q = 0; q < 4; ++q) {
        const uint4 v = src[q];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < 4; ++k)
            for (int s = 0; s < 32; s += 8) n += ((d[k] >> s) & 255u) != 0;
    }
    nonAir[b] = (uint8_t)n;
    int cubes = __popcll(w.cellMask[b]);
    for (int off = 32; off > 0; off >>= 1) cubes += __shfl_xor(cubes, off, 64);
    if (l == 0 && cubes) {
        const int mxi = (int)(m % MX), mzi = (int)((m / MX) % MZ), myi = (int)(m / ((size_t)MX * MZ));
        const int tx = (w.cx * 32 + 63) / 64, tz = (w.cz * 32 + 63) / 64;
        atomicAdd(topCount + (mxi >> 2) + tx * ((mzi >> 2) + tz * (myi >> 2)), cubes);
    }
}

}  // namespace

hipError_t launch_terrain_height(const ter::Window &t, const uint8_t *perm, float *height, hipStream_t st) {
    const size_t n = (size_t)t.cx * 32 * t.cz * 32;
    if (n == 0 || (n + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_terrain_height, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t, perm, height);
    return hipGetLastError();
}

hipError_t launch_terrain_fill(const ter::Window &t, const float *height, uint8_t *ids, hipStream_t st) {
    const size_t lanes = (size_t)t.cx * t.cy * t.cz * 2048;
    if (lanes == 0 || lanes / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_terrain_fill, dim3((unsigned)(lanes / 256)), dim3(256), 0, st, t, height, ids);
    return hipGetLastError();
}

hipError_t launch_terrain_mirrors(const WbWorld &w, uint8_t *nonAir, int *topCount, hipStream_t st) {
    const size_t nMacro = (size_t)w.cx * 2 * w.cy * 2 * w.cz * 2;
    if (nMacro == 0 || nMacro > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t nTop = (size_t)((w.cx * 32 + 63) / 64) * ((w.cy * 32 + 63) / 64) * ((w.cz * 32 + 63) / 64);
    if (hipError_t e = hipMemsetAsync(topCount, 0, nTop * sizeof(int), st)) return e;
    hipLaunchKernelGGL(k_terrain_mirrors, dim3((unsigned)nMacro), dim3(64), 0, st, w, nonAir, topCount);
    return hipGetLastError();
}

}  // namespace vx
