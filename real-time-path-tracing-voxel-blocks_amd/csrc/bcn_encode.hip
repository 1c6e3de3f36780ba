// vxpt -- the block encoders on gfx950 (bcn_encode.hpp holds the bodies, shared with the host).
//   k_bc7_encode   one wavefront per 4x4 block, four blocks per workgroup.  The 16 texels go into an LDS
//                  row of the wave once (lanes 0-15 load one each) and are read from there at
//                  wave-uniform addresses; no lane keeps them in an array.  Every lane computes the
//                  candidates that have no partition (identical across the wave), lane p those of
//                  two-subset partition p (its subset mask: one load from kBc7Part2); the winner is
//                  the wave-wide minimum of (error << 32 | ordinal) by __shfl_xor, and the lowest lane
//                  holding it writes the 16 bytes with one 128-bit store.
//   k_bc45_encode  one thread per channel block (BC5: two per block).  The search is some 30 endpoint
//                  pairs of 16 x 8 distances each: too small to split across lanes.
// Both take a job list -- per block the source level's first texel, its width, the block's x / y and
// the destination byte offset -- so that every level of every texture of a format is one launch.
#include "bcn_encode.hpp"
#include "vx_internal.hpp"

namespace vx {
namespace {

using namespace bcn;

constexpr int kThreads = 256, kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void k_bc7_encode(const uint32_t *texels, const BcEncJob *jobs, int n, int quality,
                                                         uint8_t *out) {
    __shared__ uint32_t sPx[kWaves][16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int job = blockIdx.x * kWaves + wave;
    const bool live = job < n;  // wave-uniform: the last workgroup's tail
    BcEncJob j{};
    if (live) {
        j = jobs[job];
        if (lane < 16)
            sPx[wave][lane] = texels[(size_t)j.src + (size_t)(j.by * 4u + (unsigned)(lane >> 2)) * j.width + j.bx * 4u + (unsigned)(lane & 3)];
    }
    __syncthreads();
    if (!live) return;
    const uint32_t *px = sPx[wave];
    enc::Best best;
    if (quality == 0) {
        enc::encode_bc7_fast(px, best.w);
        best.err = 0u;
        best.ord = 0u;
    } else {
        const bool opaque = enc::block_opaque(px);
        enc::bc7_shared_candidates(px, opaque, best);
        enc::bc7_partition_candidates(px, lane, opaque, best);
    }
    const uint64_t key = best.key();
    uint64_t kmin = key;
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor(kmin, d, 64);
        kmin = o < kmin ? o : kmin;
    }
    const uint64_t holders = __ballot(key == kmin);
    if (lane == __ffsll((unsigned long long)holders) - 1)
        *reinterpret_cast<uint4 *>(out + j.dst) = make_uint4(best.w[0], best.w[1], best.w[2], best.w[3]);
}

__global__ __launch_bounds__(kThreads) void k_bc45_encode(const uint32_t *texels, const BcEncJob *jobs, int n, int channels,
                                                          int quality, uint8_t *out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n * channels) return;
    const int job = channels == 2 ? i >> 1 : i, c = channels == 2 ? i & 1 : 0;
    const BcEncJob j = jobs[job];
    uint32_t px[16];
#pragma unroll
    for (int t = 0; t < 16; ++t)
        px[t] = texels[(size_t)j.src + (size_t)(j.by * 4u + (unsigned)(t >> 2)) * j.width + j.bx * 4u + (unsigned)(t & 3)];
    const uint64_t bits = enc::encode_bc4(px, c, quality);
    *reinterpret_cast<uint2 *>(out + j.dst + 8 * c) = make_uint2((uint32_t)bits, (uint32_t)(bits >> 32));
}

}  // namespace

hipError_t launch_bc_encode(int format, const uint32_t *texels, const BcEncJob *jobs, int n, int quality, uint8_t *out,
                            hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (format == kBc7) {
        hipLaunchKernelGGL(k_bc7_encode, dim3((n + kWaves - 1) / kWaves), dim3(kThreads), 0, st, texels, jobs, n, quality, out);
    } else {
        const int ch = format == kBc5 ? 2 : 1;
        hipLaunchKernelGGL(k_bc45_encode, dim3((n * ch + kThreads - 1) / kThreads), dim3(kThreads), 0, st, texels, jobs, n, ch,
                           quality, out);
    }
    return hipGetLastError();
}

}  // namespace vx
