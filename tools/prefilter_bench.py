"""Timings of the denoiser's hit-distance reconstruction and pre-pass blur on one MI355X (experiment
tool, GPU box).

python tools/prefilter_bench.py [--out profiles/NAME.json] [--calls 20] [--warmup 5] [--frames 6]

Kernels one at a time at 1920x1080 on a C3 frame (bench.py's scene, 4 spp, two frames rendered so that
the planes are a steady frame's): passes 15 and 16 through vxpt_denoise_pass, each call timed by its own
HIP events (vxpt_timings' denoise_ms), CALLS calls after WARMUP, the radiance re-uploaded before every
call so that each one filters the same input.  Each time is printed beside the pass's algorithmic bytes
and their rate as a fraction of the 8 TB/s HBM peak, in the form of bench.py's denoiser roofline:
  reconstruction  36 B read (normal 16, radiance 16, depth 4) + 16 B written per pixel
  pre-pass        centre 40 B (depth 4, material 4, normal 16, radiance 16) + 16 B written per pixel; its
                  eight taps lie within 30 pixels and are counted as cache hits
  pre-pass from the radiance itself: + the copy to the ping plane, 16 B read + 16 B written
Then the chain: vxpt_render_frames over FRAMES frames with both switches off, each alone and both on,
the mean chain time (denoise_ms) of each."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-path-tracing-voxel-blocks_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, as bench.py
W, H, SPP = 1920, 1080, 4


def c3_renderer(vxpt):
    import bench
    chunks, hs, fd, gy, pos = bench.scene_args(argparse.Namespace(scene="c3", world=256))
    r = vxpt.Renderer(W, H)
    r.load_settings()
    r.generate_terrain(chunks, height_scale=hs, freq_den=fd, global_y=gy)
    r.set_camera(pos, bench.C1_DIR, 90.0, prev=(pos, bench.C1_DIR, 90.0))
    r.set_sky()
    return r


def time_passes(vxpt, calls, warmup):
    r = c3_renderer(vxpt)
    rows = []
    try:
        p = vxpt.DenoiseParams.defaults()
        for f in range(2):
            r.render_frame(f, SPP, p)
        it = 2 * SPP
        # the planes the passes read: the last trace's radiance (1 spp planes hold the G-buffer either way)
        r.trace_flags(it, 0)
        illum = r.read("ILLUM")
        n = W * H
        cases = (("k_hitdist", 15, 0, 0, (36 + 16) * n),
                 ("k_prepass (from ping)", 16, it, 1, (40 + 16) * n),
                 ("k_copy4 + k_prepass (from illum)", 16, it, 0, (40 + 16 + 32) * n))
        for name, which, arg, arg2, alg in cases:
            ms = []
            for k in range(warmup + calls):
                r.write("ILLUM", illum)
                r.denoise_pass(which, arg, arg2, p)
                if k >= warmup:
                    ms.append(r.timings()["denoise_ms"])
            ms.sort()
            med = ms[len(ms) // 2]
            gbs = alg / (med * 1e-3) / 1e9
            rows.append({"kernel": name, "size": [W, H], "calls": calls, "warmup": warmup, "ms_median": round(med, 4),
                         "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                         "roofline": {"bound": "hbm", "kernel": name, "algorithmic_bytes": alg, "achieved": round(gbs, 1),
                                      "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                                      "ms_at_peak": round(alg / HBM_PEAK_GBS / 1e6, 4)}})
            print("%-34s %.4f ms (min %.4f, max %.4f)  %.1f MB  %.1f GB/s = %.3f of %.0f GB/s" % (
                name, med, ms[0], ms[-1], alg / 1e6, gbs, gbs / HBM_PEAK_GBS, HBM_PEAK_GBS), flush=True)
    finally:
        r.close()
    return rows


def time_chains(vxpt, frames):
    rows = []
    for recon, pre in ((0, 0), (1, 0), (0, 1), (1, 1)):
        r = c3_renderer(vxpt)
        try:
            p = vxpt.DenoiseParams.defaults()
            p.enable_hit_distance_reconstruction, p.enable_pre_pass = recon, pre
            r.render_frames(0, 2, SPP, p)  # warm-up, and frame 0's shorter chain
            r.render_frames(2, frames, SPP, p)
            t = r.timings()
            rows.append({"enable_hit_distance_reconstruction": recon, "enable_pre_pass": pre, "frames": frames,
                         "spp": SPP, "chain_ms": round(t["denoise_ms"], 4), "frame_ms": round(t["frame_ms"], 4)})
            print("chain, reconstruction %d pre-pass %d: %.4f ms (frame %.4f ms)" % (recon, pre, t["denoise_ms"],
                                                                                   t["frame_ms"]), flush=True)
        finally:
            r.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=6)
    a = ap.parse_args()
    import vxpt
    res = {"what": "k_hitdist / k_prepass one at a time at %dx%d on a C3 frame (HIP events, median of %d calls after %d), "
                   "and the denoiser chain with the switches (vxpt_render_frames, %d spp)" % (W, H, a.calls, a.warmup, SPP),
           "kernels": time_passes(vxpt, a.calls, a.warmup), "chains": time_chains(vxpt, a.frames)}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
