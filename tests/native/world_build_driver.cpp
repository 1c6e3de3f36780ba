// CPU driver of csrc/world_build.hpp (tests/test_world_build.py): the host twin of the device build on
// a world read from a file, checked here against the library's sequential construction -- the
// octant sweep S = 1 + min(S of the 7 forward neighbours) and box_tables.hpp's BrickPrefix / grow_box
// -- and written out for the test to compare with vxpt_world_tables_host.
//   world_build_driver <ids.bin> <cx> <cy> <cz> <cap> <capUp> <out.bin>
// out.bin: octant tables (8 nB u8), box tables (8 nB u32), cell masks (nB u64), sky top (4 BX BZ u16)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "box_tables.hpp"
#include "world_build.hpp"

using namespace vx;

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    const int cx = std::atoi(argv[2]), cy = std::atoi(argv[3]), cz = std::atoi(argv[4]);
    const int cap = std::atoi(argv[5]), capUp = std::atoi(argv[6]);
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> ids((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (cx <= 0 || cy <= 0 || cz <= 0 || ids.size() != (size_t)cx * cy * cz * 32768) return 2;
    const int BX = cx * 8, BY = cy * 8, BZ = cz * 8;
    const size_t nB = (size_t)BX * BY * BZ;
    std::vector<uint8_t> od(8 * nB), bricks(nB * 64);
    std::vector<uint32_t> box(8 * nB);
    std::vector<uint64_t> cell(nB), macro(nB / 64);
    std::vector<uint16_t> sky((size_t)4 * BX * BZ);
    wb::tables_host(ids.data(), cx, cy, cz, cap, capUp, bricks.data(), cell.data(), macro.data(), od.data(), box.data(),
                    sky.data());

    // the sequential construction
    long bad = 0;
    BrickPrefix P;
    P.build(BX, BY, BZ, [&](int x, int y, int z) { return cell[wb::brick_lin(BX, BZ, x, y, z)] != 0; });
    std::vector<uint8_t> S(nB);
    for (int oct = 0; oct < 8; ++oct) {
        const int sx = (oct & 1) ? 1 : -1, sy = (oct & 2) ? 1 : -1, sz = (oct & 4) ? 1 : -1;
        auto get = [&](int x, int y, int z) -> int {
            if (x < 0 || y < 0 || z < 0 || x >= BX || y >= BY || z >= BZ) return 255;
            return S[wb::brick_lin(BX, BZ, x, y, z)];
        };
        for (int iy = 0; iy < BY; ++iy)
            for (int iz = 0; iz < BZ; ++iz)
                for (int ix = 0; ix < BX; ++ix) {
                    const int x = sx > 0 ? BX - 1 - ix : ix, y = sy > 0 ? BY - 1 - iy : iy, z = sz > 0 ? BZ - 1 - iz : iz;
                    const size_t b = wb::brick_lin(BX, BZ, x, y, z);
                    int v = 0;
                    if (!cell[b]) {
                        int mn = 255;
                        for (int k = 1; k < 8; ++k)
                            mn = std::min(mn, get(x + ((k & 1) ? sx : 0), y + ((k & 2) ? sy : 0), z + ((k & 4) ? sz : 0)));
                        v = std::min(255, 1 + mn);
                    }
                    S[b] = (uint8_t)v;
                }
        for (int y = 0; y < BY; ++y)
            for (int z = 0; z < BZ; ++z)
                for (int x = 0; x < BX; ++x) {
                    const size_t b = wb::brick_lin(BX, BZ, x, y, z);
                    if (od[oct * nB + b] != S[b]) {
                        if (bad++ < 5) std::printf("cube oct %d brick %d %d %d: %d, sweep %d\n", oct, x, y, z, od[oct * nB + b], S[b]);
                    }
                    const uint32_t want = grow_box(P, x, y, z, oct, S[b], cap, capUp);
                    if (box[oct * nB + b] != want) {
                        if (bad++ < 5) std::printf("box oct %d brick %d %d %d: %x, grow_box %x\n", oct, x, y, z, box[oct * nB + b], want);
                    }
                }
    }
    std::ofstream o(argv[7], std::ios::binary);
    o.write((const char *)od.data(), od.size());
    o.write((const char *)box.data(), box.size() * 4);
    o.write((const char *)cell.data(), cell.size() * 8);
    o.write((const char *)sky.data(), sky.size() * 2);
    std::printf("mismatches %ld\n", bad);
    return bad ? 1 : 0;
}
