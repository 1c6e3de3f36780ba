"""Cost of building and editing the world's DDA tables on one MI355X: vxpt_set_world_build host (the
default, the parent's path: tests/test_gpu_world_build.py shows the two modes bit-equal) against device,
on the C3 world (256^3 cells, 64^3 bricks).  Experiment tool, GPU box.

python tools/world_build_bench.py [--out profiles/world_build.json] [--calls 9] [--warmup 2] [--frames 16]

1. vxpt_upload_voxels of the C3 ids: wall ms per call (both modes wait for the build), and the device
   build's kernels by HIP events (vxpt_world_build_ms).
2. Edits: wall ms of the call alone (`call`), of the call and the vxpt_sync after it (`synced`: when the
   tables are complete), and the kernels' HIP-event time the device path adds to the stream.
   flip: a cube set in / removed from an empty brick in mid-air at the world's centre (the brick turns
   occupied / empty: the tables behind it are redone); keep: a cube id changed in an occupied brick;
   batch64: 64 cells in 64 air bricks set, then cleared, in one vxpt_set_blocks.
3. The tables of an edit's bounded range against the whole grid (what a box-cap change launches): the
   HIP-event times that decide whether the range is kept.
4. FRAMES C3 frames (1920x1080, 4 spp, vxpt_render_frame), wall ms per frame over the loop ended by one
   vxpt_sync: the world fixed; one flipping edit before every frame in host mode; the same in device mode."""
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
FLIP = (130, 250, 130)  # mid-air at the centre: bricks behind it in all 8 octants


def c3_renderer(vxpt, mode):
    import bench
    chunks, hs, fd, gy, pos = bench.scene_args(argparse.Namespace(scene="c3", world=256))
    r = vxpt.Renderer(W, H)
    r.load_settings()
    r.set_world_build(mode)
    r.generate_terrain(chunks, height_scale=hs, freq_den=fd, global_y=gy)
    r.set_camera(pos, bench.C1_DIR, 90.0, prev=(pos, bench.C1_DIR, 90.0))
    r.set_sky()
    return r, chunks


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def timed(r, fn, calls, warmup, events):
    call, synced, ev = [], [], []
    for k in range(warmup + calls):
        r.sync()
        t0 = time.perf_counter()
        fn(k)
        t1 = time.perf_counter()
        r.sync()
        t2 = time.perf_counter()
        if k >= warmup:
            call.append((t1 - t0) * 1e3)
            synced.append((t2 - t0) * 1e3)
            if events:
                ev.append(r.world_build_ms())
    out = {"call": stats(call), "synced": stats(synced), "calls": calls, "warmup": warmup}
    if events:
        out["event_ms"] = stats(ev)
    return out


def idx(chunks, x, y, z):
    return ((x >> 5) + chunks[0] * ((z >> 5) + chunks[2] * (y >> 5))) * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    a = ap.parse_args()
    import vxpt
    res = {"what": "world tables built and edited on the host (the default, the parent's path, bit-equal to the device "
                   "path by tests/test_gpu_world_build.py) against the device, C3 world 256^3; wall ms and HIP-event ms",
           "upload_voxels": {}, "edits": {}, "frames": {}}
    for mode in ("host", "device"):
        r, chunks = c3_renderer(vxpt, mode)
        dev = mode == "device"
        try:
            ids = r.read("VOXELS").copy()
            assert not ids[idx(chunks, *FLIP)], "the flip cell is not air"
            # an occupied brick: the first cube cell of the grid, its id toggled between two cube ids
            keep_i = int(np.flatnonzero((ids >= 1) & (ids <= 12))[0])
            ch, rem = divmod(keep_i, 32768)
            keep = ((ch % chunks[0]) * 32 + rem % 32, (ch // (chunks[0] * chunks[2])) * 32 + rem // 1024,
                    (ch // chunks[0] % chunks[2]) * 32 + rem // 32 % 32)
            assert idx(chunks, *keep) == keep_i
            rng = np.random.default_rng(1)
            cells = np.stack([rng.permutation(60)[:8].repeat(8) * 4 + 8, np.full(64, 252), np.tile(rng.permutation(60)[:8], 8) * 4 + 8], 1)
            assert not any(ids[idx(chunks, *(int(v) for v in c))] for c in cells), "batch cells are not air"
            res["upload_voxels"][mode] = timed(r, lambda k: r.upload_voxels(ids, chunks), max(3, a.calls // 3), 1, dev)
            e = res["edits"][mode] = {}
            e["flip"] = timed(r, lambda k: r.set_block(*FLIP, 3 if k % 2 == 0 else 0), a.calls * 2, a.warmup * 2, dev)
            e["keep"] = timed(r, lambda k: r.set_block(*keep, 3 + k % 2), a.calls * 2, a.warmup * 2, dev)
            e["batch64"] = timed(r, lambda k: r.set_blocks(cells, np.full(64, 5 if k % 2 == 0 else 0)), a.calls * 2,
                                 a.warmup * 2, dev)
            if dev:
                whole = timed(r, lambda k: r.set_tuning(box_cap=32 - k % 2), a.calls, a.warmup, True)
                r.set_tuning(box_cap=32)
                res["range_against_whole"] = {
                    "kept": "bounded range",
                    "flip_edit_event_ms (scatter, prefix counts, tables of the range)": e["flip"]["event_ms"],
                    "whole_grid_tables_event_ms (tables kernel alone)": whole["event_ms"]}
            for kind in ("fixed", "edit"):
                for f in range(2):
                    r.render_frame(f, SPP)
                r.sync()
                t0 = time.perf_counter()
                for f in range(a.frames):
                    if kind == "edit":
                        r.set_block(*FLIP, 3 if f % 2 == 0 else 0)
                    r.render_frame(2 + f, SPP)
                r.sync()
                ms = (time.perf_counter() - t0) * 1e3 / a.frames
                res["frames"]["%s_%s" % (mode, kind)] = {"frames": a.frames, "spp": SPP, "wall_ms_per_frame": round(ms, 4)}
            print(mode, json.dumps({k: res[k].get(mode) for k in ("upload_voxels", "edits")}), flush=True)
        finally:
            r.close()
    print(json.dumps(res["frames"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
