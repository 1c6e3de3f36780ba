// vxpt -- render scale on gfx950: the frame traced below the output size is brought up to it
// (upscale.hpp holds the per-pixel bodies, shared with the host).
//   mode 0  k_bicubic             Catmull-Rom, 16 edge-clamped taps read through the cache
//   mode 1  k_easu                the edge-adaptive upsampler on a 64x16 output tile
//   mode 2  k_easu, k_sharpen     the upsampler into a second image, then the sharpener out of place
// The reference runs the upsampler and the sharpener as two full-frame passes over a half-float
// surface, the second in place (a race between neighbouring threads).  Mode 2 keeps two passes but
// sharpens out of place.  A fused kernel (the tile with a 1-pixel apron upsampled into LDS, sharpened
// from there) was built and measured 7-8 % slower at 3840x2160: the kernels are bound by
// their IEEE divisions, not by memory, the apron costs a quarter more upsampler work, and the image
// between the passes is served by the Infinity Cache.
//
// A tile stages its input footprint once, edge-clamped, as four SoA planes (R, G, B and the
// upsampler's luminance): the twelve taps of neighbouring lanes are then neighbouring or equal
// dwords of one plane row (conflict-free ds_read_b32, equal addresses broadcast).  Scale factors
// are >= 1, so E consecutive outputs anchor at most E + 1 distinct texels (E, plus one where the
// fp32 position rounds across a texel border) and the footprint is at most E + 4 wide.
#include <vector>

#include "upscale.hpp"

namespace vx {
namespace {

using namespace upscale;

constexpr int TX = 64, TY = 16, kThreads = 256;
constexpr int FW = TX + 4, FH = TY + 4;  // input footprint of a tile

struct LdsTex {
    const float *r, *g, *b, *l;
    int o;
    VX_D V3 rgb(int dx, int dy) const {
        const int k = o + dy * FW + dx;
        return V3(r[k], g[k], b[k]);
    }
    VX_D float lum(int dx, int dy) const { return l[o + dy * FW + dx]; }
};

__global__ __launch_bounds__(kThreads) void k_bicubic(const float4 *in, int W, int H, float4 *out, int OW, int OH) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= OW || y >= OH) return;
    float fx, fy;
    HostTex t{(const float *)in, W, H, 0, 0};
    t.x = bicubic_anchor(x, OW, W, fx);
    t.y = bicubic_anchor(y, OH, H, fy);
    const V3 c = bicubic(t, fx, fy);
    out[(size_t)y * OW + x] = make_float4(c.x, c.y, c.z, 0.0f);
}

__global__ __launch_bounds__(kThreads) void k_easu(const float4 *in, int W, int H, float4 *out, int OW, int OH, Map m) {
    __shared__ float sR[FH * FW], sG[FH * FW], sB[FH * FW], sL[FH * FW];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * TX, oy0 = blockIdx.y * TY;
    // the footprint: one texel before the first anchor to two past the last (anchors are monotone)
    float fr;
    const int fx0 = easu_anchor(ox0, m.sx, m.bx, fr) - 1;
    const int fy0 = easu_anchor(oy0, m.sy, m.by, fr) - 1;
    const int fw = min(easu_anchor(min(ox0 + TX, OW) - 1, m.sx, m.bx, fr) + 2 - fx0 + 1, FW);
    const int fh = min(easu_anchor(min(oy0 + TY, OH) - 1, m.sy, m.by, fr) + 2 - fy0 + 1, FH);
    for (int i = tid; i < fh * fw; i += kThreads) {
        const int ly = i / fw, lx = i - ly * fw;
        const float4 v = in[(size_t)clampi(fy0 + ly, 0, H - 1) * W + clampi(fx0 + lx, 0, W - 1)];
        const int k = ly * FW + lx;
        sR[k] = v.x;
        sG[k] = v.y;
        sB[k] = v.z;
        sL[k] = easu_lum(V3(v.x, v.y, v.z));
    }
    __syncthreads();
    for (int i = tid; i < TY * TX; i += kThreads) {
        const int ty = i / TX, tx = i - ty * TX;
        const int gx = ox0 + tx, gy = oy0 + ty;
        if (gx >= OW || gy >= OH) continue;
        float px, py;
        const int ax = easu_anchor(gx, m.sx, m.bx, px);
        const int ay = easu_anchor(gy, m.sy, m.by, py);
        // 1 <= anchor - origin <= extent - 3 by the footprint above; the clamp keeps a tap inside the planes
        const LdsTex t{sR, sG, sB, sL, clampi(ay - fy0, 1, FH - 3) * FW + clampi(ax - fx0, 1, FW - 3)};
        const V3 c = easu(t, px, py);
        out[(size_t)gy * OW + gx] = make_float4(c.x, c.y, c.z, 0.0f);
    }
}

// 64-wide rows: the 3x3 taps are coalesced row reads served by the cache
__global__ __launch_bounds__(kThreads) void k_sharpen(const float4 *in, float4 *out, int W, int H, float sharpness) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const V3 c = sharpen(HostTex{(const float *)in, W, H, x, y}, sharpness);
    out[(size_t)y * W + x] = make_float4(c.x, c.y, c.z, 0.0f);
}

}  // namespace

hipError_t launch_upscale(const float4 *in, int W, int H, float4 *out, float4 *tmp, int outW, int outH, int mode,
                          float sharpness, hipStream_t st) {
    const Map m = make_map(W, H, outW, outH);
    const dim3 tiles((outW + TX - 1) / TX, (outH + TY - 1) / TY), rows((outW + 63) / 64, (outH + 3) / 4);
    if (mode == kBicubic) {
        hipLaunchKernelGGL(k_bicubic, rows, dim3(kThreads), 0, st, in, W, H, out, outW, outH);
    } else if (mode == kEasu) {
        hipLaunchKernelGGL(k_easu, tiles, dim3(kThreads), 0, st, in, W, H, out, outW, outH, m);
    } else if (mode == kEasuSharpen) {
        hipLaunchKernelGGL(k_easu, tiles, dim3(kThreads), 0, st, in, W, H, tmp, outW, outH, m);
        hipLaunchKernelGGL(k_sharpen, rows, dim3(kThreads), 0, st, (const float4 *)tmp, out, outW, outH, sharpness);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

void upscale_host(const float *in, int w, int h, float *out, int ow, int oh, int mode, float sharpness) {
    const Map m = make_map(w, h, ow, oh);
    auto put = [](float *img, int W, int x, int y, V3 c) {
        float *p = img + 4 * ((size_t)y * W + x);
        p[0] = c.x; p[1] = c.y; p[2] = c.z; p[3] = 0.0f;
    };
    if (mode == kBicubic) {
        for (int y = 0; y < oh; ++y)
            for (int x = 0; x < ow; ++x) {
                float fx, fy;
                HostTex t{in, w, h, 0, 0};
                t.x = bicubic_anchor(x, ow, w, fx);
                t.y = bicubic_anchor(y, oh, h, fy);
                put(out, ow, x, y, bicubic(t, fx, fy));
            }
        return;
    }
    std::vector<float> tmp;
    float *up = out;
    if (mode == kEasuSharpen) {
        tmp.resize((size_t)ow * oh * 4);
        up = tmp.data();
    }
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            float px, py;
            HostTex t{in, w, h, 0, 0};
            t.x = easu_anchor(x, m.sx, m.bx, px);
            t.y = easu_anchor(y, m.sy, m.by, py);
            put(up, ow, x, y, easu(t, px, py));
        }
    if (mode != kEasuSharpen) return;
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) put(out, ow, x, y, sharpen(HostTex{up, ow, oh, x, y}, sharpness));
}

}  // namespace vx
