"""Render-scale timings on one MI355X (experiment tool, GPU box).

python tools/upscale_bench.py [--out profiles/NAME.json] [--calls 20] [--warmup 5] [--end-to-end]

Times vxpt_upscale from its own HIP events (vxpt_upscale_info) for 1920x1080 -> 3840x2160 and
2560x1440 -> 3840x2160 in each mode, CALLS calls after WARMUP, and prints each time beside its
algorithmic bytes (the input read once + the output written once, 16 B per pixel each) and their rate
as a fraction of the 8 TB/s HBM peak, in the form of bench.py's denoiser roofline.  The frame is a
fixed-seed image uploaded to VXPT_BUF_FRAME: the kernels' time does not depend on a scene.

--end-to-end adds the figure a user of the render scale sees: the C3 frame (bench.py's scene, 4 spp)
rendered at 1920x1080, post-processed and upscaled to 3840x2160 with the sharpener, against the same
frame rendered and post-processed at 3840x2160, both as host time per frame over STEPS frames
(frame-by-frame calls, synchronised at the end)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-path-tracing-voxel-blocks_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, as bench.py
SIZES = (((1920, 1080), (3840, 2160)), ((2560, 1440), (3840, 2160)))
MODES = ((0, "bicubic"), (1, "easu"), (2, "easu-sharp"))


def time_upscales(vxpt, calls, warmup):
    rows = []
    for (w, h), (ow, oh) in SIZES:
        r = vxpt.Renderer(w, h)
        try:
            img = np.random.default_rng(7).random((h, w, 4), dtype=np.float32)
            r.write("FRAME", img)
            for mode, name in MODES:
                ms = []
                for k in range(warmup + calls):
                    r._chk(r.lib.vxpt_upscale(r.ctx, ow, oh, mode, 1.0), "vxpt_upscale")
                    t = r.upscale_info()[2]
                    if k >= warmup:
                        ms.append(t)
                ms.sort()
                med = ms[len(ms) // 2]
                alg = 16 * (w * h + ow * oh)
                gbs = alg / (med * 1e-3) / 1e9
                row = {"in": [w, h], "out": [ow, oh], "mode": name, "calls": calls, "warmup": warmup,
                       "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                       "roofline": {"bound": "hbm", "kernel": "vxpt_upscale " + name, "algorithmic_bytes": alg,
                                    "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": round(gbs / HBM_PEAK_GBS, 4)}}
                rows.append(row)
                print("%dx%d -> %dx%d %-10s %.4f ms (min %.4f, max %.4f)  %.1f MB  %.1f GB/s = %.3f of %.0f GB/s" % (
                    w, h, ow, oh, name, med, ms[0], ms[-1], alg / 1e6, gbs, gbs / HBM_PEAK_GBS, HBM_PEAK_GBS), flush=True)
        finally:
            r.close()
    return rows


def end_to_end(vxpt, steps, warmup):
    import bench

    a = argparse.Namespace(scene="c3", world=256)
    chunks, hs, fd, gy, pos = bench.scene_args(a)
    params = vxpt.DenoiseParams.defaults()

    def frame_ms(w, h, upscale_to):
        r = vxpt.Renderer(w, h)
        try:
            r.load_settings()
            r.generate_terrain(chunks, height_scale=hs, freq_den=fd, global_y=gy)
            r.set_camera(pos, bench.C1_DIR, 90.0, prev=(pos, bench.C1_DIR, 90.0))
            r.set_sky()
            post = r.post_params()
            up_ms = []

            def step(f):
                r.render_frame(f, 4, params)
                r.postprocess(post, 16.6667)
                if upscale_to:
                    r._chk(r.lib.vxpt_upscale(r.ctx, upscale_to[0], upscale_to[1], 2, 1.0), "vxpt_upscale")

            for f in range(warmup):
                step(f)
            r.sync()
            t0 = time.perf_counter()
            for f in range(warmup, warmup + steps):
                step(f)
                if upscale_to:
                    up_ms.append(r.upscale_info()[2])
            r.sync()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            return round(ms, 4), (round(sorted(up_ms)[len(up_ms) // 2], 4) if up_ms else None)
        finally:
            r.close()

    # alternate the two versions (measuring-on-mi355x: compare in one call, alternating)
    scaled, native = [], []
    for _ in range(2):
        scaled.append(frame_ms(1920, 1080, (3840, 2160)))
        native.append(frame_ms(3840, 2160, None))
    res = {"what": "C3 frame (4 spp, render_frame + postprocess per frame, host time per frame over %d frames after "
                   "%d warm-up, two alternating runs each): 1920x1080 with the mode-2 upscale to 3840x2160 against "
                   "the native 3840x2160 frame" % (steps, warmup),
           "scaled_ms_per_frame": [s[0] for s in scaled], "scaled_upscale_ms_median": [s[1] for s in scaled],
           "native_ms_per_frame": [n[0] for n in native]}
    res["ratio"] = round(min(res["scaled_ms_per_frame"]) / min(res["native_ms_per_frame"]), 4)
    print("end to end: 1080p + upscale %s ms, native 4K %s ms per frame (ratio of the minima %.3f)" % (
        res["scaled_ms_per_frame"], res["native_ms_per_frame"], res["ratio"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--steps", type=int, default=10, help="--end-to-end: timed frames per run")
    a = ap.parse_args()
    import torch
    import vxpt

    if not torch.cuda.is_available():
        sys.exit("upscale_bench: no GPU (timings are taken on the device only)")
    res = {"tool": "tools/upscale_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around each vxpt_upscale (vxpt_upscale_info), median of the timed calls",
           "upscale": time_upscales(vxpt, a.calls, a.warmup)}
    if a.end_to_end:
        res["end_to_end"] = end_to_end(vxpt, a.steps, 8)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
