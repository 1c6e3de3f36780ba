"""Cost of lantern edits: host instance mode against device mode (vxpt_set_instance_build, DESIGN.md
§9.5) on the C3 world (256^3 cells) with N lanterns on the terrain surface.  Experiment tool, GPU box.

Configurations, interleaved round by round (each in a fresh process, so that none inherits another's
allocations): the parent commit's library in host mode (--parent-dir: a directory with that commit's
libvxpt.so and vxpt.py; left out when absent), this tree in host mode, device instance mode with the
host world build, device instance mode with the device world build.

Per configuration and N:
1. one lantern edit (remove / re-add in turn): wall ms of the call, wall ms until the GPU has finished,
   and in device mode the HIP-event time of the refresh (vxpt_instance_build_ms);
2. a vxpt_set_blocks batch of 64 lantern edits: the same;
3. FRAMES C3 frames (1920x1080, 4 spp, vxpt_render_frame) with one lantern edit before every frame, wall ms
   per frame over the loop ended by one sync; and the same loop with no edit.
Medians and ranges over all rounds go to --out as JSON.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "real-time-path-tracing-voxel-blocks_amd")
W, H, SPP = 1920, 1080, 4
LIGHT = 16
CONFIGS = ("parent_host", "host", "device_hostworld", "device_deviceworld")


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "n": len(ms)}


def column_tops(ids, chunks, xs, zs):
    """1 + the highest cube cell (ids 1..12) of each column (x, z); 0 for an empty column."""
    hy = chunks[1] * 32
    y = np.arange(hy)[None, :]
    x, z = xs[:, None], zs[:, None]
    i = ((x >> 5) + chunks[0] * ((z >> 5) + chunks[2] * (y >> 5))) * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))
    cube = (ids[i] >= 1) & (ids[i] <= 12)
    return np.where(cube.any(1), hy - np.argmax(cube[:, ::-1], 1), 0)


def worker(a):
    pkg = a.pkg or PKG
    for p in (REPO, pkg):
        sys.path.insert(0, p)
    import vxpt  # first: the package given by --pkg, whatever bench puts on the path
    import bench
    device = a.config.startswith("device")
    chunks, hs, fd, gy, pos = bench.scene_args(argparse.Namespace(scene="c3", world=256))
    r = vxpt.Renderer(W, H, data_dir=os.path.join(REPO, "data"))  # --pkg may lie elsewhere
    r.load_settings()
    if a.config == "device_deviceworld":
        r.set_world_build("device")
    if device:
        r.set_instance_build("device")
    r.generate_terrain(chunks, height_scale=hs, freq_den=fd, global_y=gy)
    ids = r.read("VOXELS").copy()
    rng = np.random.default_rng(7)
    cols = rng.permutation(chunks[0] * 32 * chunks[2] * 32)[:4 * a.lanterns]
    xs, zs = cols % (chunks[0] * 32), cols // (chunks[0] * 32)
    top = column_tops(ids, chunks, xs, zs)
    ok = (top > 0) & (top < chunks[1] * 32)
    cells = np.stack([xs[ok], top[ok], zs[ok]], 1)[:a.lanterns].astype(np.int32)
    assert len(cells) == a.lanterns, len(cells)
    for x, y, z in cells:
        ids[((x >> 5) + chunks[0] * ((z >> 5) + chunks[2] * (y >> 5))) * 32768 + (x & 31) + 32 * ((z & 31) + 32 * (y & 31))] = LIGHT
    r.upload_voxels(ids, chunks)
    assert r.load_models(a.models) >= 1
    assert len(r.lights()[0]) == a.lanterns
    r.set_camera(pos, bench.C1_DIR, 90.0, prev=(pos, bench.C1_DIR, 90.0))
    r.set_sky()
    r.sync()
    present = np.ones(len(cells), bool)

    def toggle(ks):
        ids_ = np.where(present[ks], 0, LIGHT)
        present[ks] = ~present[ks]
        return cells[ks], ids_

    def timed(fn, calls, warmup):
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
                if device:
                    ev.append(r.instance_build_ms())
        return {"call": call, "synced": synced, "event": ev}

    def one(k):
        c, b = toggle(np.array([k % len(cells)]))
        r.set_block(int(c[0][0]), int(c[0][1]), int(c[0][2]), int(b[0]))

    def batch(k):
        c, b = toggle(np.arange(64) % len(cells) if len(cells) < 64 else (np.arange(64) + 64 * k) % len(cells))
        r.set_blocks(c, b)

    out = {"edit": timed(one, a.edits, 2), "batch64": timed(batch, a.batches, 1)}
    p = r.denoise_params()
    for name, edit in (("frame_fixed", False), ("frame_edit", True)):
        for f in range(2):
            r.render_frame(f, SPP, p)
        r.sync()
        t0 = time.perf_counter()
        for f in range(a.frames):
            if edit:
                one(f)
            r.render_frame(2 + f, SPP, p)
        r.sync()
        out[name] = [(time.perf_counter() - t0) * 1e3 / a.frames]
    if device:
        out["stats"] = [int(v) for v in r.instance_build_stats()]
    r.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 8192])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--edits", type=int, default=10, help="single edits per round")
    ap.add_argument("--batches", type=int, default=10, help="batches of 64 per round (device mode)")
    ap.add_argument("--host-batches", type=int, default=2, help="batches of 64 per round (host mode)")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--config", default="host")
    ap.add_argument("--lanterns", type=int, default=64)
    ap.add_argument("--pkg", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    configs = [c for c in CONFIGS if c != "parent_host" or (a.parent_dir and os.path.isdir(a.parent_dir))]
    raw = {}
    for n in a.sizes:
        for rnd in range(a.rounds):
            for cfg in configs:
                env = dict(os.environ)
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--config", cfg, "--lanterns", str(n),
                       "--models", a.models, "--edits", str(a.edits), "--frames", str(a.frames),
                       "--batches", str(a.batches if cfg.startswith("device") else a.host_batches)]
                if cfg == "parent_host":
                    env["VXPT_LIB"] = os.path.join(os.path.abspath(a.parent_dir), "libvxpt.so")
                    cmd += ["--pkg", os.path.abspath(a.parent_dir)]
                res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
                if res.returncode != 0 or not line:
                    raise SystemExit("worker %s n=%d failed:\n%s\n%s" % (cfg, n, res.stdout[-2000:], res.stderr[-2000:]))
                got = json.loads(line[0][7:])
                slot = raw.setdefault((cfg, n), {})
                for k, v in got.items():
                    if k == "stats":
                        slot[k] = v
                    elif isinstance(v, dict):
                        for kk, vv in v.items():
                            slot.setdefault(k + "_" + kk, []).extend(vv)
                    else:
                        slot.setdefault(k, []).extend(v)
                print("round %d %s n=%d done" % (rnd, cfg, n), flush=True)
    result = {"what": "lantern edits on the C3 world 256^3, 1920x1080 4 spp; wall ms (call: the call alone; synced: "
                      "until the GPU is idle) and, in device mode only, HIP-event ms of the refresh on the stream "
                      "(vxpt_instance_build_ms: copies from the staging block + kernels); host mode has no such "
                      "timer, its GPU work lies inside the waits of the call, so edit_event / batch64_event are null "
                      "there.  Medians and ranges over all rounds, n = the samples behind each figure (host-mode "
                      "batches of 64 are few: --host-batches per round); frame_fixed / frame_edit: one per-frame "
                      "mean of a loop of frames_per_loop frames per round.  Configurations interleaved, one "
                      "process each; parent_host = the parent commit's library",
              "rounds": a.rounds, "frames_per_loop": a.frames, "results": []}
    for (cfg, n), slot in raw.items():
        row = {"config": cfg, "lanterns": n}
        for k, v in slot.items():
            row[k] = v if k == "stats" else (stats(v) if v else None)
        result["results"].append(row)
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
