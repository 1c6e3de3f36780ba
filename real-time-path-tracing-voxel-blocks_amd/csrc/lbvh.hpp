// vxpt -- a linear BVH over the instanced blocks (the device-mode TLAS), its
// per-element bodies shared by the host twin (vxpt_lbvh_host) and the kernels in instances.hip.
//
// Input: n primitives, each a box (lo xyz, hi xyz) and a key below 2^35 -- for an instance the 30-bit
// Morton code of its cell (10 bits per axis) above its 5-bit object index.  The primitives are sorted
// by key << 29 | index: distinct words whatever the keys, so the order is one order (for distinct
// keys, as the instance set's (cell, object) pairs are, it is the key order).  Over the sorted words
// the topology is Karras' radix tree ("Maximizing Parallelism in the Construction of BVHs, Octrees,
// and k-d Trees", HPG 2012): inner node i covers the range of words that share the longest common
// prefix around position i and splits it at the highest differing bit.  With distinct keys that bit
// lies in the key, so the depth is at most 35 (kBvhMaxDepth = 40 bounds the walk's stack).
//
// Output: the BvhNode layout of build_bvh, 2n - 1 nodes.  Node 0 is the root; inner node i keeps its
// two children at 1 + 2i and 2 + 2i (leaf or inner alike), so `left` = 1 + 2i and count = 0; a leaf
// holds one primitive: count = 1, left = its position in the sorted order.  n = 1 is one leaf root.
// Boxes: a node's box is the exact min / max union of its primitives' boxes, widened ONCE by
// 1e-4 (1 + |coordinate|) as build_bvh widens; the exact unions travel bottom-up in a buffer of their
// own, so that min / max make every box independent of the order in which children finish.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "vx_internal.hpp"

#if defined(__HIPCC__)
#define LB_HD __host__ __device__ inline
#else
#define LB_HD inline
#endif

namespace vx {
namespace lbvh {

constexpr int kKeyBits = 35, kIndexBits = 29;
constexpr uint64_t kIndexMask = ((uint64_t)1 << kIndexBits) - 1;
constexpr int kMaxN = 1 << 28;
// cells per axis a 10-bit Morton coordinate holds: a larger world keeps the host builder
constexpr int kMaxAxisCells = 1024;

LB_HD bool world_fits(int wx, int wy, int wz) { return wx <= kMaxAxisCells && wy <= kMaxAxisCells && wz <= kMaxAxisCells; }

// 10 bits -> every third bit
LB_HD uint32_t spread10(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
LB_HD uint64_t instance_key(int x, int y, int z, int object) {
    const uint32_t m = spread10((uint32_t)x) | (spread10((uint32_t)y) << 1) | (spread10((uint32_t)z) << 2);
    return ((uint64_t)m << 5) | (uint64_t)(object & 31);
}
LB_HD uint64_t pack(uint64_t key, uint32_t index) { return (key << kIndexBits) | index; }

LB_HD int clz64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return v ? __builtin_clzll(v) : 64;
#endif
}
// common prefix length of sorted words i and j; -1 outside the array
LB_HD int delta(const uint64_t *s, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    return clz64(s[i] ^ s[j]);
}

// inner node i of n - 1 (n >= 2): its children.  A child c >= 0 is inner node c, c < 0 is leaf ~c.
LB_HD void inner_children(const uint64_t *s, int n, int i, int &left, int &right) {
    const int d = delta(s, n, i, i + 1) - delta(s, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = delta(s, n, i, i - d);
    int lmax = 2;
    while (delta(s, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (delta(s, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(s, n, i, j);
    int sp = 0;
    for (int t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (delta(s, n, i, i + (sp + t) * d) > dnode) sp += t;
        if (t <= 1) break;
    }
    const int g = i + sp * d + (d < 0 ? -1 : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    left = lo == g ? ~g : g;
    right = hi == g + 1 ? ~(g + 1) : g + 1;
}

LB_HD float widen_lo(float v) { return v - 1e-4f * (1.0f + fabsf(v)); }
LB_HD float widen_hi(float v) { return v + 1e-4f * (1.0f + fabsf(v)); }
// the node of an exact box (6 floats)
LB_HD BvhNode make_node(const float *e, int left, int count) {
    BvhNode nd;
    for (int k = 0; k < 3; ++k) {
        nd.lo[k] = widen_lo(e[k]);
        nd.hi[k] = widen_hi(e[k + 3]);
    }
    nd.left = left;
    nd.count = count;
    return nd;
}
LB_HD void unite(const float *a, const float *b, float *out) {
    for (int k = 0; k < 3; ++k) {
        out[k] = a[k] < b[k] ? a[k] : b[k];
        out[k + 3] = a[k + 3] > b[k + 3] ? a[k + 3] : b[k + 3];
    }
}

// host side: the whole construction, sequential.  nodes: 2n - 1 (one zero node for n = 0 is the
// caller's business), order[k] = the primitive at sorted position k.  false: a key of 2^35 or more,
// or n out of range
inline bool build_host(const float *boxes, const uint64_t *keys, int n, BvhNode *nodes, int32_t *order) {
    if (n < 0 || n > kMaxN || (n > 0 && (!boxes || !keys || !nodes || !order))) return false;
    if (n == 0) return true;
    std::vector<uint64_t> s(n);
    for (int i = 0; i < n; ++i) {
        if (keys[i] >> kKeyBits) return false;
        s[i] = pack(keys[i], (uint32_t)i);
    }
    std::sort(s.begin(), s.end());
    for (int k = 0; k < n; ++k) order[k] = (int32_t)(s[k] & kIndexMask);
    if (n == 1) {
        nodes[0] = make_node(boxes, 0, 1);
        return true;
    }
    std::vector<int> slotInner(n - 1, 0), slotLeaf(n, 0), visits(n - 1, 0);
    for (int i = 0; i < n - 1; ++i) {
        int l, r;
        inner_children(s.data(), n, i, l, r);
        (l < 0 ? slotLeaf[~l] : slotInner[l]) = 1 + 2 * i;
        (r < 0 ? slotLeaf[~r] : slotInner[r]) = 2 + 2 * i;
    }
    std::vector<float> exact((size_t)(2 * n - 1) * 6);
    for (int k = 0; k < n; ++k) {
        int slot = slotLeaf[k];
        const float *b = boxes + (size_t)order[k] * 6;
        for (int a = 0; a < 6; ++a) exact[(size_t)slot * 6 + a] = b[a];
        nodes[slot] = make_node(b, k, 1);
        while (slot != 0) {
            const int p = (slot - 1) >> 1;
            if (visits[p]++ == 0) break;  // the second child to arrive goes on
            slot = slotInner[p];
            float *e = &exact[(size_t)slot * 6];
            unite(&exact[(size_t)(1 + 2 * p) * 6], &exact[(size_t)(2 + 2 * p) * 6], e);
            nodes[slot] = make_node(e, 1 + 2 * p, 0);
        }
    }
    return true;
}

}  // namespace lbvh
}  // namespace vx
