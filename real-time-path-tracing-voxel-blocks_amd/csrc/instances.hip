// vxpt -- the instanced blocks' TLAS built on gfx950 (vxpt_set_instance_build): a
// linear BVH over the instances that have a mesh.  The per-element bodies are lbvh.hpp's, shared with
// the host twin (vxpt_lbvh_host); the two agree bit for bit: the sort is of distinct words, the
// topology is integer work, and every node's box is a min / max union widened once.
#include "vx_internal.hpp"
#include "lbvh.hpp"

namespace vx {
namespace {

constexpr int kSortThreads = 1024;
constexpr int kSortTile = 2048;  // words one workgroup sorts in LDS (16 KiB)

// One thread per sort slot: mesh instance m < n gets its world box (the block's BLAS root box moved by
// the cell, as build_tlas computes it) and its sort word; the slots up to the padded size get the
// largest word.
__global__ __launch_bounds__(256) void k_inst_prepare(LbvhDev a) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= a.npad) return;
    if (m >= a.n) {
        a.packed[m] = ~0ull;
        return;
    }
    const int4 r = a.meshRow[a.miRow[m]];
    const BvhNode root = a.blas[a.blasRoot[r.w].x];
    const float cell[3] = {(float)r.x, (float)r.y, (float)r.z};
    float *b = a.primBox + (size_t)m * 6;
    for (int k = 0; k < 3; ++k) {
        b[k] = root.lo[k] + cell[k];
        b[k + 3] = root.hi[k] + cell[k];
    }
    a.packed[m] = lbvh::pack(lbvh::instance_key(r.x, r.y, r.z, r.w - 1), (uint32_t)m);
}

// compare-exchange t of a bitonic step (k, j): elements i and i + j, ascending where (i & k) == 0
__device__ inline int pair_low(int t, int j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// The steps that stay inside a tile of T <= kSortTile words, in LDS: for k = kStart .. kEnd, the
// sub-steps j = min(k, T) / 2 .. 1.  One workgroup per tile.
__global__ __launch_bounds__(kSortThreads) void k_bitonic_tile(uint64_t *d, int T, int kStart, int kEnd) {
    __shared__ uint64_t sh[kSortTile];
    const size_t base = (size_t)blockIdx.x * T;
    for (int t = threadIdx.x; t < T; t += kSortThreads) sh[t] = d[base + t];
    __syncthreads();
    for (int k = kStart; k <= kEnd; k <<= 1) {
        for (int j = (k < T ? k : T) >> 1; j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < (T >> 1); t += kSortThreads) {
                const int i = pair_low(t, j);
                const bool asc = ((base + i) & (size_t)k) == 0;
                const uint64_t x = sh[i], y = sh[i + j];
                if ((x > y) == asc) {
                    sh[i] = y;
                    sh[i + j] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < T; t += kSortThreads) d[base + t] = sh[t];
}

// one step whose partners lie in different tiles, in global memory; N / 2 threads
__global__ __launch_bounds__(256) void k_bitonic_step(uint64_t *d, int half, int k, int j) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= half) return;
    const int i = pair_low(t, j);
    const bool asc = (i & k) == 0;
    const uint64_t x = d[i], y = d[i + j];
    if ((x > y) == asc) {
        d[i] = y;
        d[i + j] = x;
    }
}

// Karras' radix tree over the sorted words, one thread per inner node: the node slot of each child
__global__ __launch_bounds__(256) void k_lbvh_topology(LbvhDev a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (a.n == 1) {
        if (i == 0) a.slotLeaf[0] = 0;
        return;
    }
    if (i >= a.n - 1) return;
    if (i == 0) a.slotInner[0] = 0;
    int l, r;
    lbvh::inner_children(a.packed, a.n, i, l, r);
    if (l < 0) a.slotLeaf[~l] = 1 + 2 * i; else a.slotInner[l] = 1 + 2 * i;
    if (r < 0) a.slotLeaf[~r] = 2 + 2 * i; else a.slotInner[r] = 2 + 2 * i;
}

// One thread per leaf: the sorted MeshInst, the leaf node, then upward.  At every inner node the first
// child to arrive stops and the second goes on with the union: its acquire-release add on the node's
// visit counter (agent scope) publishes this thread's exact box and makes the sibling's visible.
__global__ __launch_bounds__(256) void k_lbvh_boxes(LbvhDev a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n) return;
    const int m = (int)(a.packed[k] & lbvh::kIndexMask);
    const int row = a.miRow[m];
    const int4 r = a.meshRow[row];
    a.inst[k] = MeshInst{{(float)r.x, (float)r.y, (float)r.z}, r.w, row};
    int slot = a.slotLeaf[k];
    float e[6];
    for (int c = 0; c < 6; ++c) e[c] = a.primBox[(size_t)m * 6 + c];
    for (int c = 0; c < 6; ++c) a.exact[(size_t)slot * 6 + c] = e[c];
    a.nodes[slot] = lbvh::make_node(e, k, 1);
    while (slot != 0) {
        const int p = (slot - 1) >> 1;
        if (__hip_atomic_fetch_add(a.visits + p, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
        float x[6], y[6];
        for (int c = 0; c < 6; ++c) {
            x[c] = a.exact[(size_t)(1 + 2 * p) * 6 + c];
            y[c] = a.exact[(size_t)(2 + 2 * p) * 6 + c];
        }
        lbvh::unite(x, y, e);
        slot = a.slotInner[p];
        for (int c = 0; c < 6; ++c) a.exact[(size_t)slot * 6 + c] = e[c];
        a.nodes[slot] = lbvh::make_node(e, 1 + 2 * p, 0);
    }
}

}  // namespace

int lbvh_padded(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

hipError_t launch_lbvh_build(const LbvhDev &a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    const int N = a.npad;
    hipLaunchKernelGGL(k_inst_prepare, dim3((N + 255) / 256), dim3(256), 0, st, a);
    if (N > 1) {
        // up to kSortTile words: one workgroup, all in LDS; above: tiles sorted in LDS, then per
        // doubling the steps across tiles in global memory and the rest of the merge in LDS again
        const int T = N < kSortTile ? N : kSortTile;
        hipLaunchKernelGGL(k_bitonic_tile, dim3(N / T), dim3(kSortThreads), 0, st, a.packed, T, 2, T);
        for (int k = 2 * T; k <= N && k > 0; k <<= 1) {
            for (int j = k >> 1; j >= T; j >>= 1)
                hipLaunchKernelGGL(k_bitonic_step, dim3((N / 2 + 255) / 256), dim3(256), 0, st, a.packed, N / 2, k, j);
            hipLaunchKernelGGL(k_bitonic_tile, dim3(N / T), dim3(kSortThreads), 0, st, a.packed, T, k, k);
        }
    }
    if (a.n > 1) {
        hipError_t e = hipMemsetAsync(a.visits, 0, (size_t)(a.n - 1) * sizeof(int), st);
        if (e != hipSuccess) return e;
    }
    const int inner = a.n > 1 ? a.n - 1 : 1;
    hipLaunchKernelGGL(k_lbvh_topology, dim3((inner + 255) / 256), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lbvh_boxes, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace vx
