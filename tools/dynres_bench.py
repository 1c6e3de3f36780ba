"""Dynamic-resolution timings on one MI355X (experiment tool, GPU box).

python tools/dynres_bench.py [--out profiles/dynres.json] [--runs 11] [--warmup 3] [--frames 10]

The scene is bench.py's C3 (256^3 world, 4 spp).  Every figure is a median of RUNS runs after WARMUP, with the
minimum and maximum beside it (the spread).

resample      one vxpt_set_render_size 1920x1080 -> 1600x900 and one back, after rendered frames: the four
              resample launches alone (HIP events, vxpt_render_size_ms) and the whole call (host clock around
              the call plus a sync: it includes the call's own wait for the idle streams).  Beside it, in the
              same process, a device-to-device copy of as many bytes as the resample reads plus writes (every
              destination record is read once from the source and written once: 2 x 288 B per pixel of the new
              size -- two live G-buffer slots of 104 B, histories 32 B, history lengths 8 B, reservoirs 40 B),
              timed with HIP events, and the ratio of the kernels to that copy.
steady_state  the C3 frame time (vxpt_render_frames, HIP events, per frame) at 1600x900 on a context created at
              1920x1080 and set to that size, against a context created at 1600x900, runs alternating.
size_scan     the C3 frame time at widths 1920, 1600, 1280 and 960 (16:9) on one context created at 1920x1080:
              the curve the controller moves along."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "real-time-path-tracing-voxel-blocks_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BYTES_PER_PIXEL = 2 * 104 + 32 + 8 + 40  # what one resize resamples at a frame boundary
FULL, SMALL = (1920, 1080), (1600, 900)
SCAN = ((1920, 1080), (1600, 900), (1280, 720), (960, 540))
SPP = 4


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "runs": len(s)}


def make(vxpt, bench, size):
    a = argparse.Namespace(scene="c3", world=256)
    chunks, hs, fd, gy, pos = bench.scene_args(a)
    r = vxpt.Renderer(*size)
    r.load_settings()
    r.generate_terrain(chunks, height_scale=hs, freq_den=fd, global_y=gy)
    r.set_camera(pos, bench.C1_DIR, 90.0, prev=(pos, bench.C1_DIR, 90.0))
    r.set_sky()
    return r


def frames_ms(r, params, frame0, n):
    r.render_frames(frame0, n, SPP, params)
    return r.timings()["frame_ms"]


def resample(vxpt, bench, torch, runs, warmup):
    r = make(vxpt, bench, FULL)
    params = vxpt.DenoiseParams.defaults()
    out = {}
    try:
        frames_ms(r, params, 0, 4)
        frame = 4
        kern = {"down": [], "up": []}
        call = {"down": [], "up": []}
        for k in range(warmup + runs):
            for name, size in (("down", SMALL), ("up", FULL)):
                r.sync()
                t0 = time.perf_counter()
                r.set_render_size(*size)
                r.sync()
                ms = (time.perf_counter() - t0) * 1e3
                if k >= warmup:
                    call[name].append(ms)
                    kern[name].append(r.render_size_ms())
                frames_ms(r, params, frame, 1)  # a frame between resizes, as in use
                frame += 1
        for name, size in (("down", SMALL), ("up", FULL)):
            nbytes = BYTES_PER_PIXEL * size[0] * size[1]
            src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            src.random_(0, 255)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            copy = []
            for k in range(warmup + runs):
                ev[0].record()
                dst.copy_(src)
                ev[1].record()
                ev[1].synchronize()
                if k >= warmup:
                    copy.append(ev[0].elapsed_time(ev[1]))
            k_st, c_st, d_st = stats(kern[name]), stats(call[name]), stats(copy)
            out[name] = {"to": list(size), "bytes_read_plus_written": 2 * nbytes, "kernels_ms": k_st, "call_ms": c_st,
                         "d2d_copy_ms": d_st, "kernels_over_copy": round(k_st["median"] / d_st["median"], 3),
                         "kernels_gb_per_s": round(2 * nbytes / (k_st["median"] * 1e-3) / 1e9, 1)}
            print("resample to %dx%d: kernels %.4f ms, call %.4f ms, copy of %.1f MB %.4f ms, ratio %.3f" % (
                size[0], size[1], k_st["median"], c_st["median"], nbytes / 1e6, d_st["median"],
                out[name]["kernels_over_copy"]), flush=True)
            del src, dst
    finally:
        r.close()
    return out


def steady_state(vxpt, bench, runs, warmup, frames):
    big, small = make(vxpt, bench, FULL), make(vxpt, bench, SMALL)
    params = vxpt.DenoiseParams.defaults()
    try:
        big.set_render_size(*SMALL)
        a, b = [], []
        for k in range(warmup + runs):  # alternating
            ta = frames_ms(big, params, k * frames, frames)
            tb = frames_ms(small, params, k * frames, frames)
            if k >= warmup:
                a.append(ta)
                b.append(tb)
        sa, sb = stats(a), stats(b)
        res = {"size": list(SMALL), "created_1920x1080_ms": sa, "created_1600x900_ms": sb,
               "difference_ms": round(sa["median"] - sb["median"], 4),
               "spread_of_the_second_ms": round(sb["max"] - sb["min"], 4)}
        print("steady state at %dx%d: resized context %.4f ms, native context %.4f ms (spread %.4f)" % (
            SMALL[0], SMALL[1], sa["median"], sb["median"], res["spread_of_the_second_ms"]), flush=True)
        return res
    finally:
        big.close()
        small.close()


def size_scan(vxpt, bench, runs, warmup, frames):
    r = make(vxpt, bench, FULL)
    params = vxpt.DenoiseParams.defaults()
    rows = []
    try:
        frame = 0
        for size in SCAN:
            r.set_render_size(*size)
            ms = []
            for k in range(warmup + runs):
                t = frames_ms(r, params, frame, frames)
                frame += frames
                if k >= warmup:
                    ms.append(t)
            rows.append({"size": list(size), "frame_ms": stats(ms)})
            print("C3 frame at %dx%d: %.4f ms" % (size[0], size[1], rows[-1]["frame_ms"]["median"]), flush=True)
    finally:
        r.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=10, help="frames per timed vxpt_render_frames run")
    a = ap.parse_args()
    import torch

    import bench
    import vxpt

    if not torch.cuda.is_available():
        sys.exit("dynres_bench: no GPU (timings are taken on the device only)")
    res = {"tool": "tools/dynres_bench.py", "device": torch.cuda.get_device_name(0), "scene": "c3, %d spp" % SPP,
           "timing": "HIP events (vxpt_render_size_ms, vxpt_timings' frame_ms, torch events around the copy); "
                     "call_ms is host time around the call and a sync; medians of RUNS runs after WARMUP",
           "resample": resample(vxpt, bench, torch, a.runs, a.warmup),
           "steady_state": steady_state(vxpt, bench, a.runs, a.warmup, a.frames),
           "size_scan": size_scan(vxpt, bench, a.runs, a.warmup, a.frames)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
