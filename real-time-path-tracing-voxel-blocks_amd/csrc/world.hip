// vxpt -- the world's DDA tables built and edited on gfx950 (vxpt_set_world_build).
// The host builds the same tables in host_world.cpp (build_occupancy, octant_fill, box_fill,
// upload_sky_top); these kernels produce them bit for bit from the chunk-major ids alone.  Integer
// work throughout: the order of the atomics and of the lanes cannot change a result.
#include "vx_internal.hpp"
#include "world_build.hpp"

namespace vx {
namespace {

// One wave64 per 16^3 macro cell, one lane per 4^3 brick (lane = the brick's bit of the macro word).
// The lane gathers its 64 cells from the chunk-major ids, a 32-bit load per row of 4 x-cells, writes
// them as the brick's 64 contiguous bytes (four 16-byte stores, one per y layer) and builds the cube
// mask; the wave's ballot of non-empty masks is the macro word.
__global__ __launch_bounds__(64) void k_wb_occupancy(WbWorld w) {
    const int MX = w.cx * 2, MZ = w.cz * 2, BX = w.cx * 8;
    const size_t m = blockIdx.x;
    const int l = threadIdx.x;
    const int mxi = (int)(m % MX), mzi = (int)((m / MX) % MZ), myi = (int)(m / ((size_t)MX * MZ));
    const int bx = mxi * 4 + (l & 3), bz = mzi * 4 + ((l >> 2) & 3), by = myi * 4 + (l >> 4);
    const int x0 = bx * 4, y0 = by * 4, z0 = bz * 4;
    // a brick lies in one chunk
    const size_t ch = (size_t)(x0 >> 5) + (size_t)w.cx * ((size_t)(z0 >> 5) + (size_t)w.cz * (size_t)(y0 >> 5));
    const uint8_t *src = w.ids + ch * 32768 + (x0 & 31);
    uint64_t mask = 0;
    uint4 *dst = reinterpret_cast<uint4 *>(w.bricks + (m * 64 + l) * 64);
    for (int yi = 0; yi < 4; ++yi) {
        uint32_t row[4];
        for (int zi = 0; zi < 4; ++zi) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(src + 32 * (((z0 + zi) & 31) + 32 * ((y0 + yi) & 31)));
            row[zi] = v;
            for (int xi = 0; xi < 4; ++xi) {
                const int id = (v >> (8 * xi)) & 255;
                if (wb::is_cube(id)) mask |= 1ull << (xi + 4 * (zi + 4 * yi));
            }
        }
        dst[yi] = make_uint4(row[0], row[1], row[2], row[3]);
    }
    w.cellMask[m * 64 + l] = mask;
    const unsigned long long word = __ballot(mask != 0);
    if (l == 0) w.macro[m] = word;
    if (mask) {
        const int top = y0 + ((63 - __clzll((long long)mask)) >> 4) + 1;  // 1 + the brick's highest cube row
        atomicMax(w.colTop + (size_t)bz * BX + bx, (uint32_t)top);
    }
}

// prefix counts, first pass: one thread per (z, y) line writes the running count of occupied bricks
// along x (the planes y = 0 and z = 0 are zero)
__global__ __launch_bounds__(256) void k_wb_prefix_x(WbWorld w) {
    const int BX = w.cx * 8, BY = w.cy * 8, BZ = w.cz * 8;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)(BZ + 1) * (BY + 1)) return;
    const int z = (int)(i % (BZ + 1)), y = (int)(i / (BZ + 1));
    int *p = w.prefix + wb::prefix_index(BX, BZ, 0, y, z);
    int run = 0;
    p[0] = 0;
    for (int x = 1; x <= BX; ++x) {
        if (y > 0 && z > 0) run += w.cellMask[wb::brick_lin(BX, BZ, x - 1, y - 1, z - 1)] != 0;
        p[x] = run;
    }
}
// the other two passes: line k of `lines` starts at (k % inner) + (k / inner) * outer and runs n
// entries `stride` apart; consecutive threads take consecutive addresses
__global__ __launch_bounds__(256) void k_wb_prefix_axis(int *p, size_t lines, size_t inner, size_t outer, size_t stride,
                                                         int n) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= lines) return;
    int *q = p + (k % inner) + (k / inner) * outer;
    int run = 0;
    for (int i = 0; i < n; ++i) {
        run += q[(size_t)i * stride];
        q[(size_t)i * stride] = run;
    }
}

// one thread per (brick of the octant's range, octant): 0 if occupied, else the cube edge by binary
// search and the box grown from it
__global__ __launch_bounds__(256) void k_wb_tables(WbWorld w, WbRanges rg) {
    const int BX = w.cx * 8, BY = w.cy * 8, BZ = w.cz * 8;
    const int oct = blockIdx.y;
    const int x0 = rg.r[oct].x0, y0 = rg.r[oct].y0, z0 = rg.r[oct].z0;
    const int nx = rg.r[oct].x1 - x0 + 1, ny = rg.r[oct].y1 - y0 + 1, nz = rg.r[oct].z1 - z0 + 1;
    if (nx <= 0 || ny <= 0 || nz <= 0) return;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)nx * ny * nz) return;
    const int x = x0 + (int)(t % nx), z = z0 + (int)((t / nx) % nz), y = y0 + (int)(t / ((size_t)nx * nz));
    if (x >= BX || y >= BY || z >= BZ || x < 0 || y < 0 || z < 0) return;
    const size_t nB = (size_t)BX * BY * BZ, b = wb::brick_lin(BX, BZ, x, y, z);
    const wb::Grid g{BX, BY, BZ, w.prefix};
    uint8_t cube;
    uint32_t box;
    wb::brick_tables(g, w.cellMask[b] != 0, x, y, z, oct, w.cap, w.capUp, w.bbox != nullptr, cube, box);
    w.bdist[(size_t)oct * nB + b] = cube;
    if (w.bbox) w.bbox[(size_t)oct * nB + b] = box;
}

// one workgroup per x / z quadrant: the column tops into the quadrant's table, then a suffix maximum
// along x (a thread per row) and along z (a thread per column).  The passes work in the table itself:
// every world size takes this one path, and a workgroup's own stores are visible to it behind a barrier
__global__ __launch_bounds__(256) void k_wb_sky_top(WbWorld w) {
    const int BX = w.cx * 8, BZ = w.cz * 8, q = blockIdx.x;
    uint16_t *t = w.skyTop + (size_t)q * BX * BZ;
    for (size_t i = threadIdx.x; i < (size_t)BX * BZ; i += 256) t[i] = (uint16_t)w.colTop[i];
    __syncthreads();
    for (int z = threadIdx.x; z < BZ; z += 256) wb::suffix_max_line(t + (size_t)z * BX, BX, 1, (q & 1) != 0);
    __syncthreads();
    for (int x = threadIdx.x; x < BX; x += 256) wb::suffix_max_line(t + x, BZ, (size_t)BX, (q & 2) != 0);
}

// an edit batch's de-duplicated stores (the host mirrors hold the final values)
__global__ __launch_bounds__(256) void k_wb_edit(WbWorld w, const WbRec *rec, WbEditCounts c) {
    size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    int seg = 0;
    while (seg < 5 && t >= c.n[seg]) t -= c.n[seg++];
    if (seg == 5) return;
    size_t at = t;
    for (int s = 0; s < seg; ++s) at += c.n[s];
    const WbRec r = rec[at];
    switch (seg) {
        case 0: w.ids[r.idx] = (uint8_t)r.val; break;
        case 1: w.bricks[r.idx] = (uint8_t)r.val; break;
        case 2: w.cellMask[r.idx] = r.val; break;
        case 3: w.macro[r.idx] = r.val; break;
        default: atomicMax(w.colTop + r.idx, (uint32_t)r.val); break;
    }
}

}  // namespace

hipError_t launch_wb_occupancy(const WbWorld &w, hipStream_t st) {
    const size_t nMacro = (size_t)w.cx * 2 * w.cy * 2 * w.cz * 2;
    if (nMacro == 0 || nMacro > 0x7fffffffu) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(w.colTop, 0, (size_t)w.cx * 8 * w.cz * 8 * 4, st)) return e;
    hipLaunchKernelGGL(k_wb_occupancy, dim3((unsigned)nMacro), dim3(64), 0, st, w);
    return hipGetLastError();
}

hipError_t launch_wb_prefix(const WbWorld &w, hipStream_t st) {
    const size_t X = (size_t)w.cx * 8 + 1, Y = (size_t)w.cy * 8 + 1, Z = (size_t)w.cz * 8 + 1;
    auto blocks = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };
    hipLaunchKernelGGL(k_wb_prefix_x, blocks(Z * Y), dim3(256), 0, st, w);
    hipLaunchKernelGGL(k_wb_prefix_axis, blocks(X * Y), dim3(256), 0, st, w.prefix, X * Y, X, X * Z, X, (int)Z);
    hipLaunchKernelGGL(k_wb_prefix_axis, blocks(X * Z), dim3(256), 0, st, w.prefix, X * Z, X * Z, (size_t)0, X * Z, (int)Y);
    return hipGetLastError();
}

hipError_t launch_wb_tables(const WbWorld &w, const WbRanges &rg, hipStream_t st) {
    size_t most = 0;
    for (int o = 0; o < 8; ++o) {
        const auto &r = rg.r[o];
        if (r.x1 < r.x0 || r.y1 < r.y0 || r.z1 < r.z0) continue;
        if (r.x0 < 0 || r.y0 < 0 || r.z0 < 0 || r.x1 >= w.cx * 8 || r.y1 >= w.cy * 8 || r.z1 >= w.cz * 8)
            return hipErrorInvalidValue;
        most = std::max(most, (size_t)(r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) * (r.z1 - r.z0 + 1));
    }
    if (most == 0) return hipSuccess;
    hipLaunchKernelGGL(k_wb_tables, dim3((unsigned)((most + 255) / 256), 8), dim3(256), 0, st, w, rg);
    return hipGetLastError();
}

hipError_t launch_wb_sky_top(const WbWorld &w, hipStream_t st) {
    hipLaunchKernelGGL(k_wb_sky_top, dim3(4), dim3(256), 0, st, w);
    return hipGetLastError();
}

hipError_t launch_wb_edit(const WbWorld &w, const WbRec *rec, const WbEditCounts &c, hipStream_t st) {
    size_t n = 0;
    for (uint32_t k : c.n) n += k;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_wb_edit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, rec, c);
    return hipGetLastError();
}

}  // namespace vx
