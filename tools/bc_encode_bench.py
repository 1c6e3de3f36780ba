#!/usr/bin/env python3
"""Cost and quality of the block encoders on the ten synthetic 1024x1024 maps of DESIGN's BC speed
table: the host encoder at quality 0 and 1 (one thread), the device encoder at quality 1 (GPU time
from vxpt_bc_encode_ms and the wall time of load_textures_bc), the RMSE per format at both
qualities, and a tiny set where upload and readback dominate.  Writes profiles/bc_encode.json.

  tools/bc_encode_bench.py [--out profiles/bc_encode.json] [--parent-lib <libvxpt.so of the parent commit>]

Timing: every figure is the median of --runs repetitions after one warm-up (the host quality-1 pass
is long and runs once); clocks are left alone.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("real-time-path-tracing-voxel-blocks_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))
import test_textures  # noqa: E402
import vxpt  # noqa: E402

FMT_OF_CH = {1: vxpt.BC4, 2: vxpt.BC5, 3: vxpt.BC7, 4: vxpt.BC7}
NCH = {1: 1, 2: 2, 3: 4, 4: 4}
# the four textured materials with ten 1024 px maps (the sizes of test_textures.TEX raised to the reference's)
TEX_1024 = {
    1: ("sand", {"albedo": ("sand_a.png", 1024, 3), "normal": ("sand_n.png", 1024, 3), "roughness": ("sand_r.png", 1024, 1)}),
    2: ("soil", {"albedo": ("soil_a.png", 1024, 4), "roughness": ("soil_r.png", 1024, 2)}),
    3: ("cliff", {"albedo": ("cliff_a.png", 1024, 3), "normal": ("cliff_n.png", 1024, 3), "metallic": ("cliff_m.png", 1024, 1)}),
    7: ("rocks", {"albedo": ("rocks_a.png", 1024, 3), "normal": ("rocks_n.png", 1024, 3)}),
}


def timed(f, runs, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bc_encode.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    tex = {b: (m, {k: (fn, a.size, ch) for k, (fn, _, ch) in kinds.items()}) for b, (m, kinds) in TEX_1024.items()}
    test_textures.TEX = tex
    root = tempfile.mkdtemp(prefix="bc_encode_bench_")
    images = test_textures.make_data_dir(root)
    levels = []  # (format, channels compared, RGBA level)
    for pth in sorted(images):
        img = images[pth]
        ch = 1 if img.ndim == 2 else img.shape[2]
        for lv in test_textures.mip_chain(img):
            levels.append((FMT_OF_CH[ch], NCH[ch], np.ascontiguousarray(lv)))
    n_blocks = sum(lv.shape[0] * lv.shape[1] // 16 for _, _, lv in levels)
    res = {"maps": len(images), "map_size": a.size, "levels": len(levels), "blocks": n_blocks, "runs": a.runs}

    def host_pass(q, keep=None, lib=None):
        for fmt, _, lv in levels:
            if lib is None:
                b = vxpt.bc_encode(fmt, lv, quality=q)
            else:
                b = np.zeros(lv.shape[0] * lv.shape[1] // 16 * vxpt.bc_bytes_per_block(fmt), np.uint8)
                assert lib.vxpt_bc_encode(fmt, ctypes.c_void_p(lv.ctypes.data), lv.shape[1], lv.shape[0], ctypes.c_void_p(b.ctypes.data)) == 0
            if keep is not None:
                keep.append(b)

    med, ts = timed(lambda: host_pass(0), a.runs)
    res["host_quality0_s"] = {"median": med, "runs": ts, "against": "this commit, one thread"}
    if a.parent_lib:
        old = ctypes.CDLL(a.parent_lib)
        med, ts = timed(lambda: host_pass(0, lib=old), a.runs)
        res["host_quality0_parent_s"] = {"median": med, "runs": ts, "against": "vxpt_bc_encode of the parent commit's library, same process"}
    blocks = {0: [], 1: []}
    host_pass(0, blocks[0])
    t = time.perf_counter()
    host_pass(1, blocks[1])
    res["host_quality1_s"] = {"median": time.perf_counter() - t, "runs": 1, "against": "this commit, one thread, one run"}
    # RMSE per format over every level's texels, in 8-bit levels
    rmse = {}
    for q in (0, 1):
        acc = {}
        for (fmt, nch, lv), b in zip(levels, blocks[q]):
            dec = vxpt.bc_decode(fmt, b, lv.shape[1] // 4, lv.shape[0] // 4)
            d = (dec[..., :nch].astype(np.float64) - lv[..., :nch]) ** 2
            key = "BC%d" % fmt if fmt != vxpt.BC7 else ("BC7 RGBA" if (lv[..., 3] != 255).any() else "BC7 RGB")
            s = acc.setdefault(key, [0.0, 0])
            s[0] += d.sum()
            s[1] += d.size
        rmse["quality%d" % q] = {k: float(np.sqrt(v[0] / v[1])) for k, v in sorted(acc.items())}
    res["rmse"] = rmse

    r = vxpt.Renderer(64, 64, data_dir=root)
    r.load_settings()
    ms = []

    def search_load():
        r.load_textures_bc(encoder="search")
        ms.append(r.bc_encode_ms())

    med, ts = timed(search_load, a.runs)
    res["device_quality1_load_wall_s"] = {"median": med, "runs": ts, "against": "load_textures_bc(encoder='search'), PNG decode and mips included"}
    res["device_quality1_kernel_ms"] = {"median": statistics.median(ms[1:]), "runs": ms[1:], "against": "vxpt_bc_encode_ms (events around the three launches)"}
    med, ts = timed(lambda: r.load_textures_bc(), a.runs)
    res["host_quality0_load_wall_s"] = {"median": med, "runs": ts, "against": "load_textures_bc() (fast encoder on the host), PNG decode and mips included"}
    # and the device blocks are the host's
    table, _ = r.texture_table_bc()
    r.load_textures_bc(encoder="search")
    dev = r.read("TEX_BLOCKS")
    k, same = 0, True
    for fmt, size, max_lod, offs in table:
        for l in range(max_lod + 1):
            same = same and (dev[offs[l]:offs[l] + blocks[1][k].size] == blocks[1][k]).all()
            k += 1
    res["device_equals_host_quality1"] = bool(same)
    # a tiny image: upload, launch and readback against the host search
    small = levels[0][2][:16, :16].copy()
    med_d, _ = timed(lambda: r.bc_encode(vxpt.BC7, small, quality=1), 20)
    med_h, _ = timed(lambda: vxpt.bc_encode(vxpt.BC7, small, quality=1), 20)
    res["tiny_16px_bc7_quality1_s"] = {"device_wall": med_d, "host_wall": med_h, "device_kernel_ms": r.bc_encode_ms()}
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
