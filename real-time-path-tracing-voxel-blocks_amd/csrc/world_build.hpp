// vxpt -- the per-brick bodies of the world's DDA tables, shared by the kernels (world.hip), the host
// twin behind vxpt_world_tables_host and the CPU test driver (tests/native/world_build_driver.cpp).
// No HIP is needed to include it.
//
// Everything here is integer work on the brick grid (BX x BY x BZ bricks of 4^3 cells), independent
// per brick and octant once the 3-D prefix counts of occupied bricks exist:
//   cube_edge   the cube tables' entry WITHOUT octant_fill's sweep.  The recurrence S = 1 + min(S of
//               the 7 forward neighbours) computes the edge of the largest empty cube cornered at the
//               brick; "the s-cube, clamped to the grid, holds no occupied brick" is monotone in s, so
//               the largest such s <= 255 is a binary search over the prefix counts (8 probes).
//   grow_box    box_tables.hpp's growth (x, then z, then y; cap / capUp; the stop at the world's edge)
//               over a plain pointer to the prefix counts.
//   sky_top     the sky-exit table: the 2-D suffix maximum of the column tops per x / z quadrant is
//               separable, a suffix maximum along x, then along z.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define WB_HD __host__ __device__
#else
#define WB_HD
#endif

namespace vx {
namespace wb {

// brick grid and its prefix counts: p has (BX + 1) x (BZ + 1) x (BY + 1) entries, index
// x + (BX + 1) * (z + (BZ + 1) * y) (box_tables.hpp BrickPrefix::p)
struct Grid {
    int BX, BY, BZ;
    const int *p;
};

WB_HD inline int imin(int a, int b) { return a < b ? a : b; }
WB_HD inline int imax(int a, int b) { return a > b ? a : b; }

// brick coordinates -> index of the cell masks and of one octant's table (16^3 macro cell, then brick)
WB_HD inline size_t brick_lin(int BX, int BZ, int bx, int by, int bz) {
    const size_t m = (size_t)(bx >> 2) + (size_t)(BX >> 2) * ((size_t)(bz >> 2) + (size_t)(BZ >> 2) * (size_t)(by >> 2));
    return m * 64 + (size_t)((bx & 3) + 4 * ((bz & 3) + 4 * (by & 3)));
}
WB_HD inline size_t prefix_size(int BX, int BY, int BZ) { return (size_t)(BX + 1) * (BY + 1) * (BZ + 1); }
WB_HD inline size_t prefix_index(int BX, int BZ, int x, int y, int z) {
    return (size_t)x + (size_t)(BX + 1) * ((size_t)z + (size_t)(BZ + 1) * (size_t)y);
}
WB_HD inline bool is_cube(int id) { return id >= 1 && id <= 12; }

// occupied bricks in [x0, x1) x [y0, y1) x [z0, z1), clamped to the grid
WB_HD inline int count(const Grid &g, int x0, int y0, int z0, int x1, int y1, int z1) {
    x0 = imax(x0, 0); y0 = imax(y0, 0); z0 = imax(z0, 0);
    x1 = imin(x1, g.BX); y1 = imin(y1, g.BY); z1 = imin(z1, g.BZ);
    if (x0 >= x1 || y0 >= y1 || z0 >= z1) return 0;
    const int *p = g.p;
    const int BX = g.BX, BZ = g.BZ;
    return p[prefix_index(BX, BZ, x1, y1, z1)] - p[prefix_index(BX, BZ, x0, y1, z1)] -
           p[prefix_index(BX, BZ, x1, y0, z1)] - p[prefix_index(BX, BZ, x1, y1, z0)] +
           p[prefix_index(BX, BZ, x0, y0, z1)] + p[prefix_index(BX, BZ, x0, y1, z0)] +
           p[prefix_index(BX, BZ, x1, y0, z0)] - p[prefix_index(BX, BZ, x0, y0, z0)];
}

// is the box of extents (ex, ey, ez) bricks at brick (x, y, z), extending into octant oct, empty?
WB_HD inline bool box_empty(const Grid &g, int x, int y, int z, int oct, int ex, int ey, int ez) {
    const int x0 = (oct & 1) ? x : x - ex + 1, x1 = (oct & 1) ? x + ex : x + 1;
    const int y0 = (oct & 2) ? y : y - ey + 1, y1 = (oct & 2) ? y + ey : y + 1;
    const int z0 = (oct & 4) ? z : z - ez + 1, z1 = (oct & 4) ? z + ez : z + 1;
    return count(g, x0, y0, z0, x1, y1, z1) == 0;
}

// the cube table's entry of an EMPTY brick: the largest s in 1..255 whose s-cube is empty
WB_HD inline int cube_edge(const Grid &g, int x, int y, int z, int oct) {
    int lo = 1, hi = 255;  // the 1-cube is the brick itself
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (box_empty(g, x, y, z, oct, mid, mid, mid)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// box_tables.hpp grow_box: the box of brick (x, y, z) in octant oct grown from its cube edge S
WB_HD inline uint32_t grow_box(const Grid &g, int x, int y, int z, int oct, int S, int cap, int capUp) {
    if (S <= 0) return 0u;
    const int b[3] = {x, y, z}, n[3] = {g.BX, g.BY, g.BZ};
    int e[3] = {S, S, S};
    const int lim = imin(255, imax(S, cap)), limUp = imin(255, imax(S, capUp));
    for (int k = 0; k < 3; ++k) {
        const int a = k == 0 ? 0 : (k == 1 ? 2 : 1);  // x, then z, then y
        const bool pos = (oct >> a) & 1;
        const int l = (a == 1 && pos) ? limUp : lim;
        while (e[a] < l) {
            // the box already reaches the world's edge on this axis: growing adds nothing
            if (pos ? b[a] + e[a] >= n[a] : b[a] - e[a] + 1 <= 0) break;
            int t[3] = {e[0], e[1], e[2]};
            ++t[a];
            if (!box_empty(g, x, y, z, oct, t[0], t[1], t[2])) break;
            e[a] = t[a];
        }
    }
    return (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
}

// one (brick, octant) entry of both tables; occupied: 0 / 0
WB_HD inline void brick_tables(const Grid &g, bool occupied, int x, int y, int z, int oct, int cap, int capUp, bool boxes,
                               uint8_t &cube, uint32_t &box) {
    cube = 0;
    box = 0u;
    if (occupied) return;
    const int S = cube_edge(g, x, y, z, oct);
    cube = (uint8_t)S;
    if (boxes) box = grow_box(g, x, y, z, oct, S, cap, capUp);
}

// sky-exit table, one line of one pass: t[i * stride] for i in 0..n-1 becomes the maximum over the
// entries at and after it in the quadrant's direction (positive: towards larger i)
template <class T>
WB_HD inline void suffix_max_line(T *t, int n, size_t stride, bool positive) {
    T m = 0;
    for (int k = 0; k < n; ++k) {
        const int i = positive ? n - 1 - k : k;
        T &v = t[(size_t)i * stride];
        if (v > m) m = v;
        v = m;
    }
}

// ---------------------------------------------------------------------------------------------
// host twin: every table of a world from its chunk-major ids (x + 32 * (z + 32 * y) per 32^3 chunk,
// chunks x-major, then z, then y), by the bodies above.  Any output may be null.
inline void tables_host(const uint8_t *ids, int cx, int cy, int cz, int cap, int capUp, uint8_t *brickIds,
                        uint64_t *cellMasks, uint64_t *macroMasks, uint8_t *octantTables, uint32_t *boxTables,
                        uint16_t *skyTop) {
    const int wx = cx * 32, wy = cy * 32, wz = cz * 32, BX = cx * 8, BY = cy * 8, BZ = cz * 8;
    const size_t nB = (size_t)BX * BY * BZ;
    std::vector<uint64_t> cell(nB, 0ull);
    std::vector<uint32_t> colTop((size_t)BX * BZ, 0u);
    if (brickIds) std::fill(brickIds, brickIds + nB * 64, (uint8_t)0);
    if (macroMasks) std::fill(macroMasks, macroMasks + nB / 64, 0ull);
    for (int y = 0; y < wy; ++y)
        for (int z = 0; z < wz; ++z)
            for (int x = 0; x < wx; ++x) {
                const size_t ch = (size_t)(x >> 5) + (size_t)cx * ((z >> 5) + (size_t)cz * (y >> 5));
                const uint8_t id = ids[ch * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))];
                if (!id) continue;
                const size_t b = brick_lin(BX, BZ, x >> 2, y >> 2, z >> 2);
                const int lc = (x & 3) + 4 * ((z & 3) + 4 * (y & 3));
                if (brickIds) brickIds[b * 64 + lc] = id;
                if (!is_cube(id)) continue;
                cell[b] |= 1ull << lc;
                if (macroMasks) macroMasks[b / 64] |= 1ull << (b % 64);
                uint32_t &ct = colTop[(size_t)(z >> 2) * BX + (x >> 2)];
                if (ct < (uint32_t)(y + 1)) ct = (uint32_t)(y + 1);
            }
    if (cellMasks) std::copy(cell.begin(), cell.end(), cellMasks);
    if (skyTop)
        for (int q = 0; q < 4; ++q) {
            uint16_t *t = skyTop + (size_t)q * BX * BZ;
            for (size_t i = 0; i < (size_t)BX * BZ; ++i) t[i] = (uint16_t)colTop[i];
            for (int z = 0; z < BZ; ++z) suffix_max_line(t + (size_t)z * BX, BX, 1, (q & 1) != 0);
            for (int x = 0; x < BX; ++x) suffix_max_line(t + x, BZ, (size_t)BX, (q & 2) != 0);
        }
    if (!octantTables && !boxTables) return;
    // prefix counts: the occupancy, then a running sum along x, along z, along y
    std::vector<int> p(prefix_size(BX, BY, BZ), 0);
    for (int y = 1; y <= BY; ++y)
        for (int z = 1; z <= BZ; ++z)
            for (int x = 1; x <= BX; ++x)
                p[prefix_index(BX, BZ, x, y, z)] = cell[brick_lin(BX, BZ, x - 1, y - 1, z - 1)] != 0;
    for (int y = 1; y <= BY; ++y)
        for (int z = 1; z <= BZ; ++z)
            for (int x = 1; x <= BX; ++x) p[prefix_index(BX, BZ, x, y, z)] += p[prefix_index(BX, BZ, x - 1, y, z)];
    for (int y = 1; y <= BY; ++y)
        for (int z = 1; z <= BZ; ++z)
            for (int x = 1; x <= BX; ++x) p[prefix_index(BX, BZ, x, y, z)] += p[prefix_index(BX, BZ, x, y, z - 1)];
    for (int y = 1; y <= BY; ++y)
        for (int z = 1; z <= BZ; ++z)
            for (int x = 1; x <= BX; ++x) p[prefix_index(BX, BZ, x, y, z)] += p[prefix_index(BX, BZ, x, y - 1, z)];
    const Grid g{BX, BY, BZ, p.data()};
    for (int oct = 0; oct < 8; ++oct)
        for (int y = 0; y < BY; ++y)
            for (int z = 0; z < BZ; ++z)
                for (int x = 0; x < BX; ++x) {
                    const size_t b = brick_lin(BX, BZ, x, y, z);
                    uint8_t cube;
                    uint32_t box;
                    brick_tables(g, cell[b] != 0, x, y, z, oct, cap, capUp, boxTables != nullptr, cube, box);
                    if (octantTables) octantTables[(size_t)oct * nB + b] = cube;
                    if (boxTables) boxTables[(size_t)oct * nB + b] = box;
                }
}

}  // namespace wb
}  // namespace vx
