// Dynamic resolution: the point resample that carries a context's histories from one render size to
// another (vxpt_set_render_size), one body for the host (vxpt_resize_host) and the device (resize.hip).
//
// New pixel (x, y) takes old pixel (sx, sy) whole: the old pixel under the new pixel's centre,
//   sx = min(((2x + 1) * oldW) / (2 * newW), oldW - 1), the same in y,
// in integers (truncating division), so that host and device agree bit for bit and no value is
// blended: a new pixel's planes are one old pixel's complete record.  Sizes are at most kResizeMaxDim,
// which keeps (2x + 1) * oldW inside 32 bits.
//
// A plane is addressed in units of T (4 or 16 bytes), PER of them per pixel: 20-byte reservoirs are
// 5 dwords, the 32-byte tap records 2 float4.  One destination unit per call, so that neighbouring
// calls store neighbouring units.
#pragma once
#include <cstddef>
#include <cstdint>

#include "vx_math.hpp"

namespace vx {
namespace resize {

constexpr int kResizeMaxDim = 32768;

struct Map {
    int oldW, oldH, newW, newH;
};

// the old index under the centre of new index d, along an axis of oldN -> newN pixels
VX_HD int src_index(int d, int oldN, int newN) {
    const uint32_t s = ((2u * (uint32_t)d + 1u) * (uint32_t)oldN) / (2u * (uint32_t)newN);
    return s < (uint32_t)oldN ? (int)s : oldN - 1;
}

// unit ex of row y of the new plane (ex < newW * PER); sy = src_index(y, oldH, newH)
template <class T, int PER>
VX_HD void resize_unit(const T *src, T *dst, const Map &m, int ex, int y, int sy) {
    const int x = ex / PER, sub = ex - x * PER;
    const int sx = src_index(x, m.oldW, m.newW);
    dst[((size_t)y * m.newW + x) * PER + sub] = src[((size_t)sy * m.oldW + sx) * PER + sub];
}

// a whole plane on the host
template <class T, int PER>
inline void resize_plane_host(const T *src, T *dst, const Map &m) {
    for (int y = 0; y < m.newH; ++y) {
        const int sy = src_index(y, m.oldH, m.newH);
        for (int ex = 0; ex < m.newW * PER; ++ex) resize_unit<T, PER>(src, dst, m, ex, y, sy);
    }
}

struct U16 {  // a 16-byte unit the host can copy too
    uint32_t v[4];
};

// bytes per pixel the library resamples: float planes, float4 planes, reservoirs, tap records
VX_HD bool bpp_ok(int bpp) { return bpp == 4 || bpp == 16 || bpp == 20 || bpp == 32; }

inline void resize_host(const void *src, void *dst, const Map &m, int bpp) {
    if (bpp == 4) resize_plane_host<uint32_t, 1>((const uint32_t *)src, (uint32_t *)dst, m);
    else if (bpp == 16) resize_plane_host<U16, 1>((const U16 *)src, (U16 *)dst, m);
    else if (bpp == 20) resize_plane_host<uint32_t, 5>((const uint32_t *)src, (uint32_t *)dst, m);
    else if (bpp == 32) resize_plane_host<U16, 2>((const U16 *)src, (U16 *)dst, m);
}

}  // namespace resize
}  // namespace vx
