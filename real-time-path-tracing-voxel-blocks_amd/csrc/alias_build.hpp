// vxpt -- a parallel alias-table construction, its bodies shared by the host twin
// (vxpt_alias_build_host) and the kernels in sky.hip (vxpt_alias_build, vxpt_set_sky_device).
//
// The table's inputs are Vose's (build_alias, host_sky.cpp): sum = (float) of a double sum of the
// weights, p[i] = w[i] / sum and s[i] = p[i] * n in binary32.  The double sum is taken in ONE fixed
// tree order (tree_sum below), the same on the host and on the device:
//   - the weights are cut into chunks of kChunk = 1024 consecutive items (the last one padded with
//     +0.0); lane t of 256 adds its 4 consecutive items 4t .. 4t+3 in index order, starting from 0.0;
//   - the chunk's 256 lane values are folded by halving: for h = 128, 64 .. 1: v[t] += v[t + h], t < h;
//   - lane t of 256 then adds the chunk sums t, t + 256, t + 512 .. in that order, starting from 0.0,
//     and the 256 lane values are folded by the same halving.
// s is then turned into 64-bit fixed point with kFracBits = 40 fraction bits, rounded to nearest
// (ties to even); an s that is not finite or above 2^22 (a zero or non-finite sum) counts as exactly 1.
// From there everything is integer, so any summation order gives the same bits:
//   - lights are the bins with s < 1, heavies those with s >= 1, both kept in index order;
//   - D_k = the sum of (1 - s) over the first k lights (D_0 = 0, k = 0 .. m),
//     E_j = the sum of (s - 1) over heavies 0 .. j;
//   - light k: q = s, alias = the heavy with the smallest j such that E_j >= D_k; none (the heavies
//     ran out, Vose's drain loop): q = 1, alias = -1;
//   - heavy j: K = the smallest index with D_K > E_j; when K exists and heavy j + 1 exists,
//     q = 1 + E_j - D_K (converted to binary32 through an exact double: one rounding) and alias =
//     heavy j + 1 (-1 when that q rounds to 1: the alias would never be taken, and alias = -1 then
//     marks exactly the bins with q = 1, as in Vose's table); otherwise q = 1, alias = -1.
// This is the two-list sweep (lights poured into the heavies in order, a heavy that drops below 1
// topped up by the next heavy) without its sequential loop: every bin does two binary searches over
// monotone arrays and depends on no other bin's result.  It does not reproduce Vose's FIFO pairing.
// n <= kMaxN = 2^22 keeps every sum below 2^63.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define AB_HD __host__ __device__ inline
#else
#define AB_HD inline
#endif

namespace vx {
namespace ab {

constexpr int kFracBits = 40;
constexpr int64_t kOne = (int64_t)1 << kFracBits;
constexpr int kLanes = 256, kPerLane = 4, kChunk = kLanes * kPerLane;
constexpr int kMaxN = 1 << 22;

AB_HD float prob(float w, float sum) { return w / sum; }
AB_HD float scaled(float p, int n) { return p * (float)(unsigned)n; }
AB_HD int64_t fixed(float s) {
    if (!(fabsf(s) <= 4194304.0f)) return kOne;
    return (int64_t)llrint((double)s * 1099511627776.0);
}
AB_HD float unfixed(int64_t v) { return (float)((double)v * (1.0 / 1099511627776.0)); }

// tree_sum's leaves: lane `lane` of chunk `chunk` over its 4 consecutive items
AB_HD double lane_sum(const float *w, int n, int chunk, int lane) {
    double a = 0.0;
    const int base = chunk * kChunk + lane * kPerLane;
    for (int k = 0; k < kPerLane; ++k) a += (base + k < n) ? (double)w[base + k] : 0.0;
    return a;
}
// lane `lane` of the second level over the chunk sums lane, lane + 256 ..
AB_HD double top_lane_sum(const double *part, int chunks, int lane) {
    double a = 0.0;
    for (int c = lane; c < chunks; c += kLanes) a += part[c];
    return a;
}

// smallest j in [0, h) with E[j] >= v (E non-decreasing); h when there is none
AB_HD int first_heavy(const int64_t *E, int h, int64_t v) {
    int lo = 0, hi = h;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (E[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// smallest K in [0, m] with D[K] > v (D[0 .. m] increasing); m + 1 when there is none
AB_HD int first_deficit(const int64_t *D, int m, int64_t v) {
    int lo = 0, hi = m + 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (D[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the two lists: D[0 .. m], E[0 .. h - 1], heavy[j] = the bin of heavy j
struct Lists {
    const int64_t *D, *E;
    const int *heavy;
    int m, h;
};
AB_HD void light_bin(const Lists &l, int k, float s, float &q, int &alias) {
    const int j = first_heavy(l.E, l.h, l.D[k]);
    if (j < l.h) { q = s; alias = l.heavy[j]; }
    else { q = 1.0f; alias = -1; }
}
AB_HD void heavy_bin(const Lists &l, int j, float &q, int &alias) {
    const int K = first_deficit(l.D, l.m, l.E[j]);
    if (K <= l.m && j + 1 < l.h) {
        q = unfixed(kOne + l.E[j] - l.D[K]);
        alias = q < 1.0f ? l.heavy[j + 1] : -1;
    } else {
        q = 1.0f; alias = -1;
    }
}

// host side: the fixed tree order and the whole construction with sequential scans
inline double fold256(double *v) {
    for (int h = kLanes / 2; h >= 1; h >>= 1)
        for (int t = 0; t < h; ++t) v[t] += v[t + h];
    return v[0];
}
inline double tree_sum(const float *w, int n) {
    const int chunks = (n + kChunk - 1) / kChunk;
    std::vector<double> part(chunks);
    double v[kLanes];
    for (int c = 0; c < chunks; ++c) {
        for (int t = 0; t < kLanes; ++t) v[t] = lane_sum(w, n, c, t);
        part[c] = fold256(v);
    }
    for (int t = 0; t < kLanes; ++t) v[t] = top_lane_sum(part.data(), chunks, t);
    return fold256(v);
}

// the host twin: the whole construction, sequential scans
inline bool build_host(const float *w, int n, float *q, float *p, int32_t *alias, float *sum) {
    if (!w || n < 1 || n > kMaxN) return false;
    const float fsum = (float)tree_sum(w, n);
    if (sum) *sum = fsum;
    std::vector<int64_t> D(1, 0), E;
    std::vector<int> light, heavy;
    std::vector<float> pv(n);
    for (int i = 0; i < n; ++i) {
        pv[i] = prob(w[i], fsum);
        const int64_t f = fixed(scaled(pv[i], n));
        if (f < kOne) {
            light.push_back(i);
            D.push_back(D.back() + (kOne - f));
        } else {
            heavy.push_back(i);
            E.push_back((E.empty() ? 0 : E.back()) + (f - kOne));
        }
    }
    const Lists l{D.data(), E.data(), heavy.data(), (int)light.size(), (int)heavy.size()};
    for (int k = 0; k < l.m; ++k) {
        const int i = light[k];
        float qq; int a;
        light_bin(l, k, scaled(pv[i], n), qq, a);
        if (q) q[i] = qq;
        if (alias) alias[i] = a;
    }
    for (int j = 0; j < l.h; ++j) {
        const int i = heavy[j];
        float qq; int a;
        heavy_bin(l, j, qq, a);
        if (q) q[i] = qq;
        if (alias) alias[i] = a;
    }
    if (p) for (int i = 0; i < n; ++i) p[i] = pv[i];
    return true;
}

}  // namespace ab
}  // namespace vx
