// CPU test driver (host code only, no kernel launch): the library's voxel walk (vx_device.hpp, host +
// device) with the pass-through of occupied bricks (dda_iter's PASS, WorldDev::brickPass) against the
// walk without it, over a world read from a chunk-major id file.  Every ray is walked with the cube
// tables and the box tables, with brickSteps 3 and unlimited, whole, through the straggler save /
// resume hand-over after 0-6 iterations and cut into 1 / 2 / 4 / 8 / 16 pieces; visibility rays are
// added whose tmin / tmax fall inside a brick the walk passes through.  Prints the rays that differ
// (hit, cell, face, id, t bits; occlusion) and what the pass-through saves: the occupied-brick
// visits it takes and the cell steps they replace.
// Usage: brick_pass_driver ids.bin CX CY CZ nrays seed
//        brick_pass_driver ids.bin CX CY CZ --cam px py pz dx dy dz fovDeg W H sunx suny sunz
//          (a pinhole camera's rays, then from each hit one cosine-weighted hemisphere ray and one ray
//          toward the sun: the counts per ray class, box tables, whole bricks)
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <random>
#include <vector>

#include "box_tables.hpp"
#include "vx_device.hpp"

using namespace vx;

namespace {

struct Count { long visits = 0, passes = 0, cells = 0, iters = 0; };

bool same_hit(const Hit &a, const Hit &b) {
    return a.hit == b.hit && a.x == b.x && a.y == b.y && a.z == b.z && a.face == b.face && a.id == b.id &&
           float_as_bits(a.t) == float_as_bits(b.t);
}
const Hit kMiss{0, 0, 0, 0, -1, 0, kRayMax};

// a whole walk; handover: every iteration through dda_save / dda_resume.  *inside: the first brick
// the walk passes through, as (t of the first crossing from the walk's cell, t of the brick's exit)
template <bool OCC, bool BOX, bool PASS>
int whole_walk(const WorldDev &w, V3 o, V3 d, float tmin, float tmax, bool handover, Hit &out, Count *c = nullptr,
               float *inside = nullptr) {
    Hit h = kMiss;
    Dda s;
    int rc = dda_begin<OCC, BOX>(w, o, d, tmin, tmax, s, h);
    bool found = false;
    while (rc == DdaRun) {
        if (handover) {
            const DdaSaved sv = dda_save(s, 0);
            dda_resume<BOX>(w, o, d, tmin, tmax, sv, s);
        }
        const bool pass = PASS && brick_passes(w, s);
        if (c) {
            c->visits += s.dist == 0;
            c->passes += pass;
            ++c->iters;
        }
        if (pass && inside && !found) {
            Cell e = s.c;
            skip_box(w, s.r, e, 1, 1, 1);
            inside[0] = fminf(s.c.tx, fminf(s.c.ty, s.c.tz));
            inside[1] = fminf(e.tx, fminf(e.ty, e.tz));
            found = true;
        }
        int cnt[5] = {0, 0, 0, 0, 0};
        rc = dda_iter<OCC, BOX, GlobalBricks, BOX, PASS>(w, s, h, c ? cnt : nullptr);
        if (c) c->cells += cnt[4];
    }
    out = rc == DdaEvent ? h : kMiss;
    if (inside && !found) inside[0] = inside[1] = -1.0f;
    return rc;
}

// the straggler hand-over after `cap` iterations, the rest cut into up to G pieces (k_resume_split)
template <bool OCC, bool PASS>
int split_walk(const WorldDev &w, V3 o, V3 d, float tmin, float tmax, int cap, int G, Hit &out) {
    Hit h = kMiss;
    Dda s;
    int rc = dda_begin<OCC, true>(w, o, d, tmin, tmax, s, h);
    for (int k = 0; rc == DdaRun && k < cap; ++k) rc = dda_iter<OCC, true, GlobalBricks, true, PASS>(w, s, h);
    if (rc != DdaRun) { out = rc == DdaEvent ? h : kMiss; return rc; }
    const DdaSaved sv = dda_save(s, 0);
    Dda s0;
    dda_resume<true>(w, o, d, tmin, tmax, sv, s0);
    int D, n;
    float te;
    const int pieces = seg_plan(w, s0, G, D, n, te);
    for (int k = 0; k < pieces; ++k) {
        Dda sk;
        dda_resume<true>(w, o, d, tmin, tmax, sv, sk);
        int P0 = 0, P1 = 0;
        const float T0 = k > 0 ? seg_bound(sk, D, k, pieces, n, P0) : 0.0f;
        const float T1 = k + 1 < pieces ? seg_bound(sk, D, k + 1, pieces, n, P1) : tmax;
        if (k > 0 && !(T0 < te)) break;
        if (k > 0) dda_seg_start<true>(w, sk, D, P0, T0);
        sk.tmax = fminf(T1, tmax);
        Hit hk = kMiss;
        int r = DdaRun;
        while (r == DdaRun) r = dda_iter<OCC, true, GlobalBricks, true, PASS>(w, sk, hk);
        if (r == DdaEvent) { out = hk; return DdaEvent; }
    }
    out = kMiss;
    return DdaNone;
}

// one ray, pass-through on against off, in every whole-walk configuration: the differences
template <bool BOX>
int whole_diffs(const WorldDev &w, V3 o, V3 d, float tmin, float tmax, bool handover) {
    Hit a, b;
    int n = 0;
    const int ra = whole_walk<false, BOX, true>(w, o, d, 0.0f, tmax, handover, a);
    const int rb = whole_walk<false, BOX, false>(w, o, d, 0.0f, tmax, handover, b);
    n += ra != rb || !same_hit(a, b);
    const int oa = whole_walk<true, BOX, true>(w, o, d, tmin, tmax, handover, a);
    const int ob = whole_walk<true, BOX, false>(w, o, d, tmin, tmax, handover, b);
    n += oa != ob;
    return n;
}

struct Worlds { WorldDev cube0, cube3, box0, box3; };

int ray_diffs(const Worlds &W, V3 o, V3 d, float tmin, float tmax, bool handover) {
    return whole_diffs<false>(W.cube0, o, d, tmin, tmax, handover) + whole_diffs<false>(W.cube3, o, d, tmin, tmax, handover) +
           whole_diffs<true>(W.box0, o, d, tmin, tmax, handover) + whole_diffs<true>(W.box3, o, d, tmin, tmax, handover);
}

V3 unit(V3 v) {
    const float l = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return V3(v.x / l, v.y / l, v.z / l);
}
V3 cross3(V3 a, V3 b) { return V3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

}  // namespace

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    const int CX = atoi(argv[2]), CY = atoi(argv[3]), CZ = atoi(argv[4]);
    const int wx = CX * 32, wy = CY * 32, wz = CZ * 32, BX = wx / 4, BY = wy / 4, BZ = wz / 4;
    std::vector<uint8_t> ids((size_t)wx * wy * wz);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(ids.data(), 1, ids.size(), f) != ids.size()) return 1;
    fclose(f);
    const size_t nB = (size_t)BX * BY * BZ;
    auto blin = [&](int bx, int by, int bz) {  // vx_device.hpp brick_index
        const size_t m = (size_t)(bx >> 2) + (size_t)(CX * 2) * ((bz >> 2) + (size_t)(CZ * 2) * (by >> 2));
        return m * 64 + (size_t)((bx & 3) + 4 * ((bz & 3) + 4 * (by & 3)));
    };
    std::vector<uint8_t> bricks(nB * 64, 0);
    std::vector<uint64_t> cellMask(nB, 0);
    const int nbx = wx / 4, nbz = wz / 4;
    std::vector<uint16_t> colTop((size_t)nbx * nbz, 0), skyTop((size_t)4 * nbx * nbz, 0);
    for (int y = 0; y < wy; ++y)
        for (int z = 0; z < wz; ++z)
            for (int x = 0; x < wx; ++x) {
                const size_t ch = (x >> 5) + (size_t)CX * ((z >> 5) + (size_t)CZ * (y >> 5));
                const uint8_t id = ids[ch * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))];
                if (!id) continue;
                const size_t b = blin(x >> 2, y >> 2, z >> 2);
                const int lc = (x & 3) + 4 * ((z & 3) + 4 * (y & 3));
                bricks[b * 64 + lc] = id;
                if (id >= 1 && id <= 12) {
                    cellMask[b] |= 1ull << lc;
                    uint16_t &ct = colTop[(size_t)(z >> 2) * nbx + (x >> 2)];
                    if (ct < y + 1) ct = (uint16_t)(y + 1);
                }
            }
    // the cube tables (the library's octant recurrence, whole grid)
    std::vector<uint8_t> od(8 * nB, 0);
    for (int oct = 0; oct < 8; ++oct) {
        uint8_t *S = od.data() + oct * nB;
        const int sx = (oct & 1) ? 1 : -1, sy = (oct & 2) ? 1 : -1, sz = (oct & 4) ? 1 : -1;
        auto get = [&](int x, int y, int z) -> int {
            if (x < 0 || y < 0 || z < 0 || x >= BX || y >= BY || z >= BZ) return 255;
            return S[blin(x, y, z)];
        };
        for (int iy = 0; iy < BY; ++iy)
            for (int iz = 0; iz < BZ; ++iz)
                for (int ix = 0; ix < BX; ++ix) {
                    const int x = sx > 0 ? BX - 1 - ix : ix, y = sy > 0 ? BY - 1 - iy : iy, z = sz > 0 ? BZ - 1 - iz : iz;
                    int v = 0;
                    if (!cellMask[blin(x, y, z)]) {
                        int mn = 255;
                        for (int k = 1; k < 8; ++k)
                            mn = std::min(mn, get(x + ((k & 1) ? sx : 0), y + ((k & 2) ? sy : 0), z + ((k & 4) ? sz : 0)));
                        v = std::min(255, 1 + mn);
                    }
                    S[blin(x, y, z)] = (uint8_t)v;
                }
    }
    // the box tables (the library's builder)
    BrickPrefix pre;
    pre.build(BX, BY, BZ, [&](int x, int y, int z) { return cellMask[blin(x, y, z)] != 0; });
    std::vector<uint32_t> box(8 * nB, 0);
    for (int oct = 0; oct < 8; ++oct)
        for (int y = 0; y < BY; ++y)
            for (int z = 0; z < BZ; ++z)
                for (int x = 0; x < BX; ++x) {
                    const size_t b = blin(x, y, z);
                    box[oct * nB + b] = grow_box(pre, x, y, z, oct, od[oct * nB + b]);
                }
    // the sky exit's table (the library's upload_sky_top, restated)
    for (int q = 0; q < 4; ++q)
        for (int kz = 0; kz < nbz; ++kz)
            for (int kx = 0; kx < nbx; ++kx) {
                const int bz = (q & 2) ? nbz - 1 - kz : kz, bx = (q & 1) ? nbx - 1 - kx : kx;
                const int fz = (q & 2) ? bz + 1 : bz - 1, fx = (q & 1) ? bx + 1 : bx - 1;
                uint16_t *t = skyTop.data() + (size_t)q * nbx * nbz;
                uint16_t m = colTop[(size_t)bz * nbx + bx];
                if (fz >= 0 && fz < nbz && t[(size_t)fz * nbx + bx] > m) m = t[(size_t)fz * nbx + bx];
                if (fx >= 0 && fx < nbx && t[(size_t)bz * nbx + fx] > m) m = t[(size_t)bz * nbx + fx];
                t[(size_t)bz * nbx + bx] = m;
            }
    WorldDev w{};
    w.bricks = bricks.data();
    w.cellMask = cellMask.data();
    w.bdist = od.data();
    w.bbox = box.data();
    w.nBricks = (int)nB;
    w.cx = CX; w.cy = CY; w.cz = CZ;
    w.wx = wx; w.wy = wy; w.wz = wz;
    w.mx = wx / 16; w.my = wy / 16; w.mz = wz / 16;
    w.brickPass = 1;
    Worlds W{w, w, w, w};  // the cube walks: no sky exit; the box walks with it, as the kernels run them
    W.cube3.brickSteps = 3;
    W.box0.skyTop = skyTop.data();
    W.box3.skyTop = skyTop.data();
    W.box3.brickSteps = 3;
    WorldDev boxOff = W.box0;  // the run-time switch off: PASS walks must take no brick then
    boxOff.brickPass = 0;

    if (std::string(argv[5]) == "--cam") {
        if (argc < 18) return 2;
        const V3 pos((float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8]));
        const V3 fwd = unit(V3((float)atof(argv[9]), (float)atof(argv[10]), (float)atof(argv[11])));
        const float th = tanf((float)atof(argv[12]) * 3.14159265f / 360.0f);
        const int IW = atoi(argv[13]), IH = atoi(argv[14]);
        const V3 sun = unit(V3((float)atof(argv[15]), (float)atof(argv[16]), (float)atof(argv[17])));
        const V3 right = unit(cross3(fwd, V3(0, 1, 0))), up = cross3(right, fwd);
        std::mt19937 rng(11);
        std::uniform_real_distribution<float> U(0.0f, 1.0f);
        Count on[3], off[3];
        long rays[3] = {0, 0, 0}, diff = 0;
        auto both = [&](int cls, V3 o, V3 d, bool occ, Hit &h) {
            Hit hb;
            int ra, rb;
            if (occ) {
                ra = whole_walk<true, true, true>(W.box0, o, d, 0.0f, 1e27f, false, h, &on[cls]);
                rb = whole_walk<true, true, false>(W.box0, o, d, 0.0f, 1e27f, false, hb, &off[cls]);
            } else {
                ra = whole_walk<false, true, true>(W.box0, o, d, 0.0f, 1e27f, false, h, &on[cls]);
                rb = whole_walk<false, true, false>(W.box0, o, d, 0.0f, 1e27f, false, hb, &off[cls]);
                diff += !same_hit(h, hb);
            }
            diff += ra != rb;
            ++rays[cls];
        };
        for (int py = 0; py < IH; ++py)
            for (int px = 0; px < IW; ++px) {
                const float u = (px + 0.5f) / IW * 2.0f - 1.0f, v = 1.0f - (py + 0.5f) / IH * 2.0f;
                const float ax = u * th * IW / IH, ay = v * th;
                const V3 d = unit(V3(fwd.x + ax * right.x + ay * up.x, fwd.y + ax * right.y + ay * up.y,
                                     fwd.z + ax * right.z + ay * up.z));
                Hit h;
                both(0, pos, d, false, h);
                if (!h.hit) continue;
                // secondary rays leave the hit face's plane, just outside the cube
                V3 n(0, 0, 0);
                if (h.face == 0) n.y = 1; else if (h.face == 1) n.y = -1; else if (h.face == 2) n.x = -1;
                else if (h.face == 3) n.x = 1; else if (h.face == 4) n.z = 1; else n.z = -1;
                const V3 p(pos.x + d.x * h.t + n.x * 1e-3f, pos.y + d.y * h.t + n.y * 1e-3f, pos.z + d.z * h.t + n.z * 1e-3f);
                const float r = sqrtf(U(rng)), phi = 6.2831853f * U(rng), cz = sqrtf(fmaxf(0.0f, 1.0f - r * r));
                const V3 t1 = fabsf(n.y) > 0.5f ? V3(1, 0, 0) : V3(0, 1, 0), t2 = cross3(n, t1);
                const float a = r * cosf(phi), b = r * sinf(phi);
                const V3 hd = unit(V3(a * t1.x + b * t2.x + cz * n.x, a * t1.y + b * t2.y + cz * n.y, a * t1.z + b * t2.z + cz * n.z));
                Hit h2;
                both(1, p, hd, false, h2);
                if (sun.x * n.x + sun.y * n.y + sun.z * n.z > 0.0f) both(2, p, sun, true, h2);
            }
        const char *names[3] = {"cam", "hemi", "sun"};
        for (int k = 0; k < 3; ++k)
            printf("%s rays %ld visits %ld passes %ld cells-off %ld cells-on %ld iters-off %ld iters-on %ld\n", names[k], rays[k],
                   off[k].visits, on[k].passes, off[k].cells, on[k].cells, off[k].iters, on[k].iters);
        printf("diff %ld\n", diff);
        return 0;
    }

    const int nrays = atoi(argv[5]);
    std::mt19937 rng((unsigned)atoi(argv[6]));
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    long diff = 0, hits = 0, splitDiff = 0, splitRuns = 0, insideRuns = 0, insideDiff = 0, offPasses = 0;
    Count on, off;
    for (int i = 0; i < nrays; ++i) {
        const bool outside = i % 4 == 0;
        V3 o(U(rng) * wx, U(rng) * wy, U(rng) * wz);
        if (outside) o = V3(o.x * 3 - wx, o.y * 3 - wy, o.z * 3 - wz);
        V3 d(U(rng) * 2 - 1, U(rng) * 2 - 1, U(rng) * 2 - 1);
        if (i % 11 == 0) d.y = 0.0f;
        if (i % 13 == 0) d.x = 0.0f;
        if (i % 17 == 0) d.z = 0.0f;
        if (i % 5 == 0) d.y = -fabsf(d.y) - 0.3f;  // toward the terrain
        if (i % 9 == 0) d.y *= 0.05f;              // low rays that graze the surface bricks
        const float len = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
        if (!(len > 0.0f)) continue;
        d = V3(d.x / len, d.y / len, d.z / len);
        const float tmax = (i % 7 == 0) ? 20.0f : 1e27f, tmin = (i % 3 == 0) ? 0.5f : 0.0f;
        // the counted pair (box tables, whole bricks) and the first passed-through brick's t range
        Hit ha, hb;
        float in[2];
        const int ra = whole_walk<false, true, true>(W.box0, o, d, 0.0f, tmax, false, ha, &on, in);
        const int rb = whole_walk<false, true, false>(W.box0, o, d, 0.0f, tmax, false, hb, &off);
        hits += hb.hit;
        int nd = (ra != rb || !same_hit(ha, hb)) ? 1 : 0;
        Count c0;
        Hit hz;
        whole_walk<false, true, true>(boxOff, o, d, 0.0f, tmax, false, hz, &c0);
        offPasses += c0.passes;
        nd += !same_hit(hz, hb);
        nd += ray_diffs(W, o, d, tmin, tmax, false) + ray_diffs(W, o, d, tmin, tmax, true);
        if (nd) {
            if (diff < 5)
                printf("diff ray %d: off hit %d (%d %d %d) f%d t %.9g | on hit %d (%d %d %d) f%d t %.9g\n", i, hb.hit, hb.x,
                       hb.y, hb.z, hb.face, hb.t, ha.hit, ha.x, ha.y, ha.z, ha.face, ha.t);
            ++diff;
        }
        // visibility rays (and a closest-hit ray) whose tmin / tmax fall inside the passed-through brick
        if (in[0] >= 0.0f && in[0] < in[1]) {
            const float mid = 0.5f * (in[0] + in[1]);
            if (mid > in[0] && mid < in[1]) {
                const float cases[4][2] = {{mid, 1e27f}, {0.0f, mid}, {in[0], mid}, {mid, in[1]}};
                for (const auto &cs : cases) {
                    ++insideRuns;
                    const int k = ray_diffs(W, o, d, cs[0], cs[1], (i & 1) != 0);
                    if (k && insideDiff < 5) printf("inside diff ray %d tmin %.9g tmax %.9g\n", i, cs[0], cs[1]);
                    insideDiff += k != 0;
                }
            }
        }
        for (int G : {1, 2, 4, 8, 16}) {
            const int cap = i % 7;
            for (const WorldDev *wp : {&W.box3, &W.box0}) {
                Hit sa, sb, so;
                const int r1 = split_walk<false, true>(*wp, o, d, 0.0f, tmax, cap, G, sa);
                const int r0 = split_walk<false, false>(*wp, o, d, 0.0f, tmax, cap, G, sb);
                const bool o1 = split_walk<true, true>(*wp, o, d, tmin, tmax, cap, G, so) == DdaEvent;
                const bool o0 = split_walk<true, false>(*wp, o, d, tmin, tmax, cap, G, so) == DdaEvent;
                ++splitRuns;
                // (and the split walk is the whole walk)
                if (r1 != r0 || !same_hit(sa, sb) || o1 != o0 || !same_hit(sa, hb)) {
                    if (splitDiff < 5)
                        printf("split diff ray %d G %d cap %d: off hit %d (%d %d %d) f%d t %.9g | on hit %d (%d %d %d) f%d t %.9g | occ %d %d\n",
                               i, G, cap, sb.hit, sb.x, sb.y, sb.z, sb.face, sb.t, sa.hit, sa.x, sa.y, sa.z, sa.face, sa.t, o0, o1);
                    ++splitDiff;
                }
            }
        }
    }
    printf("rays %d hits %ld diff %ld split-runs %ld split-diff %ld inside-runs %ld inside-diff %ld visits %ld passes %ld "
           "cells-off %ld cells-on %ld iters-off %ld iters-on %ld off-passes %ld\n",
           nrays, hits, diff, splitRuns, splitDiff, insideRuns, insideDiff, off.visits, on.passes, off.cells, on.cells,
           off.iters, on.iters, offPasses);
    return 0;
}
