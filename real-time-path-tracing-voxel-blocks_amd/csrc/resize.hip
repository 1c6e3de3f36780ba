// vxpt -- dynamic resolution on gfx950: the histories of a context resampled from the old render size to
// the new one (resize.hpp holds the body, shared with the host).
//
// One kernel shape for every record size: a lane per destination unit (a dword or a float4), a
// workgroup per 256 consecutive units of one destination row, grid.y the rows, grid.z the planes of
// the launch.  A wave's stores are 256 B / 1 KiB of consecutive bytes; its loads are runs of
// consecutive bytes too (an enlargement repeats source pixels, a reduction skips some), so the
// gather is served by whole cache lines.  The source row is uniform per workgroup; the only per-lane
// arithmetic is one 32-bit division.  Every plane of one unit type and units-per-pixel count goes
// into one launch through a table passed by value: four launches per resize (float planes, float4
// planes, tap records as 2 float4, reservoirs as 5 dwords).
#include <algorithm>

#include "resize.hpp"
#include "vx_internal.hpp"

namespace vx {
namespace {

using namespace resize;

constexpr int kThreads = 256;

template <class T, int PER>
__global__ __launch_bounds__(kThreads) void k_resize(ResizePlanes p, Map m) {
    const int ex = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
    if (ex >= m.newW * PER) return;  // (y < newH by the grid)
    const int sy = src_index(y, m.oldH, m.newH);
    resize_unit<T, PER>((const T *)p.src[blockIdx.z], (T *)p.dst[blockIdx.z], m, ex, y, sy);
}

template <class T, int PER>
hipError_t launch(const ResizePlanes &p, const Map &m, hipStream_t st) {
    if (p.n == 0) return hipSuccess;
    const dim3 grid((m.newW * PER + kThreads - 1) / kThreads, m.newH, p.n);
    hipLaunchKernelGGL((k_resize<T, PER>), grid, dim3(kThreads), 0, st, p, m);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resize(const ResizePlanes &p, int bytesPerPixel, int oldW, int oldH, int newW, int newH,
                         hipStream_t st) {
    if (p.n < 0 || p.n > kResizePlanes || oldW < 1 || oldH < 1 || newW < 1 || newH < 1 ||
        std::max(std::max(oldW, oldH), std::max(newW, newH)) > kResizeMaxDim)  // (grid.y <= 65535 with it)
        return hipErrorInvalidValue;
    const Map m{oldW, oldH, newW, newH};
    switch (bytesPerPixel) {
        case 4: return launch<uint32_t, 1>(p, m, st);
        case 16: return launch<uint4, 1>(p, m, st);
        case 20: return launch<uint32_t, 5>(p, m, st);
        case 32: return launch<uint4, 2>(p, m, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vx
