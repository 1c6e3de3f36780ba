"""Cost of generating the terrain on one MI355X, device world-build mode: vxpt_generate_terrain (host
noise and fill loops, upload, host mirrors: the parent's path, whose code this tree only moved into
csrc/terrain.hpp) against vxpt_generate_terrain_ex (kernels, mirrors read back).  tests/test_gpu_terrain.py
shows the two bit-equal.  Experiment tool, GPU box.

python tools/terrain_bench.py [--out profiles/terrain_build.json] [--runs 11] [--warmup 2] [--frames 32] [--every 8]

1. Per world -- C3 (8,8,8 chunks, 256^3 cells), C1 (2,1,2) and one chunk (1,1,1) -- wall ms per call, both
   calls wait for the GPU before they return; the two paths alternate in one process after a warm-up;
   median and range of RUNS runs.  _ex split by its HIP events (vxpt_terrain_ms: height kernel, fill
   kernel, table kernels, mirror readback); the old path split into its host generator (vxpt_terrain_host)
   and vxpt_upload_voxels, each timed alone.
2. The same _ex call on a context in host world-build mode (host generator + upload: where it cannot win).
3. FRAMES C3 frames (1920x1080, 4 spp, vxpt_render_frame), wall ms per frame over a loop ended by one
   vxpt_sync: the world fixed; regenerated every EVERY frames by vxpt_generate_terrain; regenerated every
   EVERY frames by _ex with the window moved 32 cells along x."""
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

W, H, SPP = 1920, 1080, 4
WORLDS = {"c3_8x8x8": dict(chunks=(8, 8, 8), height_scale=128.0, freq_den=256.0, global_y=True),
          "c1_2x1x2": dict(chunks=(2, 1, 2), height_scale=32.0, freq_den=64.0, global_y=False),
          "one_chunk": dict(chunks=(1, 1, 1), height_scale=32.0, freq_den=32.0, global_y=False)}


def stats(ms):
    s = sorted(float(v) for v in ms)
    return {"ms_median": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4), "runs": len(s)}


def wall(r, fn):
    r.sync()
    t0 = time.perf_counter()
    fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def world_times(vxpt, kw, runs, warmup):
    flags = 2 if kw["global_y"] else 0
    host_args = (kw["chunks"], kw["height_scale"], kw["freq_den"], flags, (0, 0, 0), 124)
    ids = vxpt.terrain_host(*host_args)
    out = {}
    r = vxpt.Renderer(64, 64)
    h = vxpt.Renderer(64, 64)
    try:
        r.load_settings()
        r.set_world_build("device")
        h.load_settings()
        t = {k: [] for k in ("generate_terrain", "ex", "host_generator", "upload_voxels", "ex_host_mode")}
        ev = []
        for k in range(warmup + runs):
            a = wall(r, lambda: r.generate_terrain(**kw))
            b = wall(r, lambda: r.generate_terrain(ex=True, **kw))
            e = r.terrain_ms()
            if k == 0:
                np.testing.assert_array_equal(r.read("VOXELS"), ids)
            c = wall(r, lambda: vxpt.terrain_host(*host_args))
            d = wall(r, lambda: r.upload_voxels(ids, kw["chunks"]))
            f = wall(h, lambda: h.generate_terrain(ex=True, **kw))
            if k >= warmup:
                for key, v in zip(t, (a, b, c, d, f)):
                    t[key].append(v)
                ev.append(e)
        out = {key: stats(v) for key, v in t.items()}
        ev = np.asarray(ev)
        out["ex_event_ms"] = {n: stats(list(ev[:, i])) for i, n in enumerate(("height", "fill", "tables", "readback"))}
        out["cells"] = int(ids.size)
        out["speedup_median"] = round(out["generate_terrain"]["ms_median"] / out["ex"]["ms_median"], 3)
    finally:
        r.close()
        h.close()
    return out


def frame_loop(vxpt, frames, every):
    import bench
    chunks, hs, fd, gy, pos = bench.scene_args(argparse.Namespace(scene="c3", world=256))
    kw = dict(chunks=chunks, height_scale=hs, freq_den=fd, global_y=gy)
    r = vxpt.Renderer(W, H)
    out = {}
    try:
        r.load_settings()
        r.set_world_build("device")
        r.generate_terrain(**kw)
        r.set_camera(pos, bench.C1_DIR, 90.0, prev=(pos, bench.C1_DIR, 90.0))
        r.set_sky()
        for kind in ("fixed", "generate_terrain", "ex_moving_window", "fixed_again"):
            for f in range(2):
                r.render_frame(f, SPP)
            r.sync()
            t0 = time.perf_counter()
            for f in range(frames):
                if f % every == 0 and kind == "generate_terrain":
                    r.generate_terrain(**kw)
                if f % every == 0 and kind == "ex_moving_window":
                    r.generate_terrain(origin=(32 * (f // every), 0, 0), ex=True, **kw)
                r.render_frame(2 + f, SPP)
            r.sync()
            out[kind] = {"frames": frames, "spp": SPP, "regenerate_every": 0 if kind.startswith("fixed") else every,
                         "wall_ms_per_frame": round((time.perf_counter() - t0) * 1e3 / frames, 4)}
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--every", type=int, default=8)
    a = ap.parse_args()
    import vxpt
    res = {"what": "terrain generated by vxpt_generate_terrain (host loops + upload + host mirrors) against "
                   "vxpt_generate_terrain_ex (kernels + mirror readback), device world-build mode, one MI355X; wall ms "
                   "of calls that wait for the GPU, alternating in one process; HIP-event ms for the split",
           "worlds": {}, "frames": {}}
    for name, kw in WORLDS.items():
        res["worlds"][name] = world_times(vxpt, kw, a.runs, a.warmup)
        print(name, json.dumps(res["worlds"][name]), flush=True)
    res["frames"] = frame_loop(vxpt, a.frames, a.every)
    print(json.dumps(res["frames"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
