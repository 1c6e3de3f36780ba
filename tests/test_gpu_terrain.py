"""The terrain generated on the device (vxpt_generate_terrain_ex in device world-build mode,
csrc/terrain.hip) against its host twin vxpt_terrain_host and against vxpt_upload_voxels of the same
ids, which stays the yardstick: ids, every table, and the host mirrors as the ABI shows them (chunk
files, picking, the nearest surface, edits), all bit-equal.
"""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import terrain_ref as T
import vxpt
from golden.make_golden import C1_CAMERA
from test_edits import EXE, REPO, STRUCTS, _idx

pytestmark = pytest.mark.gpu

TABLES = STRUCTS + ("SKY_TOP",)
PLANES = ("OUTPUT", "ILLUM", "DEPTH", "NORMAL_ROUGH", "GEO_NORMAL_THIN", "ALBEDO", "MATERIAL", "MAT_PARAM", "MOTION")
# a world with cubes, shader balls (instanced ids) and two chunk layers
MIRROR_CASE = ((2, 2, 2), 48.0, 64.0, T.GLOBAL_Y | T.BALLS, (3, 0, 11), 5)


def _renderer(mode="device"):
    r = vxpt.Renderer(64, 48)
    r.load_settings()
    r.set_world_build(mode)
    return r


def _ex(r, case):
    chunks, hs, fd, flags, origin, seed = case
    r.generate_terrain(chunks, height_scale=hs, freq_den=fd, keep_shader_balls=bool(flags & T.BALLS),
                       global_y=bool(flags & T.GLOBAL_Y), origin=origin, seed=seed, ex=True)


_HOST = {}


def _host(case):
    if case not in _HOST:
        _HOST[case] = vxpt.terrain_host(*case)
    return _HOST[case]


def _uploaded(case, mode="device"):
    r = _renderer(mode)
    r.upload_voxels(_host(case), case[0])
    return r


def _assert_same(a, b, what=""):
    for name in TABLES:
        np.testing.assert_array_equal(a.read(name), b.read(name), err_msg="%s %s" % (name, what))


@pytest.mark.parametrize("case", T.CASES, ids=str)
def test_device_ids_equal_the_host_twin(case):
    r = _renderer()
    _ex(r, case)
    np.testing.assert_array_equal(r.read("VOXELS"), _host(case))
    r.close()


def test_the_256_cube_world_equals_the_host_twin():
    case = ((8, 8, 8), 128.0, 256.0, T.GLOBAL_Y, (0, 0, 0), 124)
    r = _renderer()
    _ex(r, case)
    ids = r.read("VOXELS")
    np.testing.assert_array_equal(ids, _host(case))
    assert 0 < np.count_nonzero(ids) < ids.size
    r.close()


@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("case", [T.CASES[1], T.CASES[5], MIRROR_CASE], ids=str)
def test_tables_equal_an_upload_of_the_same_ids(case, mode):
    a, b = _renderer(mode), _uploaded(case, mode)
    _ex(a, case)
    _assert_same(a, b)
    a.close()
    b.close()


def _pick_rays(n, chunks, seed):
    rng = np.random.default_rng(seed)
    ext = np.array(chunks, np.float64) * 32
    pos = rng.uniform(-0.2, 1.2, (n, 3)) * ext
    pos[:, 1] = rng.uniform(0.3, 1.3, n) * ext[1]
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1])
    return pos, d / np.linalg.norm(d, axis=1, keepdims=True)


def test_host_mirrors_equal_an_upload_of_the_same_ids(tmp_path):
    case = MIRROR_CASE
    chunks = case[0]
    a, b = _renderer(), _uploaded(case)
    _ex(a, case)
    # chunk files are written from the mirror of the chunk-major ids
    # (named by their hash; the scene file lists the hash of every chunk)
    for r, name in ((a, "a"), (b, "b")):
        r.set_camera([10.0, 50.0, 10.0], [0.0, -1.0, 0.0], 90.0)
        r.save_world(tmp_path / (name + ".yaml"), tmp_path / name)
    files = sorted(os.listdir(tmp_path / "b"))
    assert len(files) > 1 and sorted(os.listdir(tmp_path / "a")) == files
    assert filecmp.cmp(tmp_path / "a.yaml", tmp_path / "b.yaml", shallow=False)
    for f in files:
        assert filecmp.cmp(tmp_path / "a" / f, tmp_path / "b" / f, shallow=False), f
    # picking walks the mirrors: the 64^3 block word, the macro and cell masks, the ids
    pos, d = _pick_rays(200, chunks, 9)
    hits = 0
    for p, v in zip(pos, d):
        for r in (a, b):
            r.set_camera(list(p), list(v), 90.0)
        pa, pb = a.pick_block(), b.pick_block()
        assert pa == pb, (p, v)
        hits += pa["hit"]
    assert 10 < hits
    # the nearest surface reads the per-brick non-air counts
    for p in np.concatenate([pos[:40], [[10.5, 90.0, 10.5], [40.0, 7.5, 54.5]]]):
        assert a.nearest_surface(list(p)) == b.nearest_surface(list(p)), p
    # edits update the mirrors in place: bricks emptied and filled, columns raised, an instanced id
    ids = _host(case)
    rng = np.random.default_rng(4)
    edits = [(8 + i % 4, 4 + (i // 4) % 4, 20 + i // 16, 0) for i in range(16)]      # cells of one brick, emptied
    edits += [(50, 62, 50, 3), (51, 62, 50, 16), (50, 62, 50, 0), (5, 63, 5, 7)]     # empty air: filled, emptied, raised
    while len(edits) < 32:
        x, y, z = (int(rng.integers(0, 64)) for _ in range(3))
        edits.append((x, y, z, int(rng.choice([0, 1, 12, 16]))))
    assert ids[_idx(8, 4, 20, chunks)] != 0 and ids[_idx(50, 62, 50, chunks)] == 0
    e = np.asarray(edits, np.int32)
    for r in (a, b):
        r.set_blocks(e[:16, :3], e[:16, 3])
        r.set_blocks(e[16:, :3], e[16:, 3])
    _assert_same(a, b, "after edits")
    for p, v in zip(pos[:50], d[:50]):
        for r in (a, b):
            r.set_camera(list(p), list(v), 90.0)
        assert a.pick_block() == b.pick_block()
    a.close()
    b.close()


def test_regeneration_on_one_context():
    r = _renderer()
    steps = [((2, 1, 2), 32.0, 64.0, 0, (0, 0, 0), 124), ((1, 1, 1), 32.0, 32.0, T.BALLS, (20, 0, 20), 124),
             ((2, 2, 2), 48.0, 64.0, T.GLOBAL_Y, (-64, 0, 7), 99)]
    for case in steps:
        _ex(r, case)
        fresh = _uploaded(case)
        _assert_same(r, fresh, str(case))
        np.testing.assert_array_equal(r.read("VOXELS"), _host(case))
        r.set_camera([16.5, 40.0, 16.5], [0.1, -1.0, 0.05], 90.0)
        fresh.set_camera([16.5, 40.0, 16.5], [0.1, -1.0, 0.05], 90.0)
        assert r.pick_block() == fresh.pick_block()
        fresh.close()
    r.close()


def _frames(ex):
    r = _renderer()
    r.generate_terrain((2, 1, 2), ex=ex)
    r.set_camera(C1_CAMERA[0], C1_CAMERA[1], fov=C1_CAMERA[2], prev=C1_CAMERA)
    r.set_sky()
    dp = r.denoise_params()
    out = []
    for f in range(2):
        r.render_frame(f, 1, dp)
        out.append([r.read(n) for n in PLANES])
    r.close()
    return out


def test_frames_after_ex_equal_frames_after_generate_terrain():
    old, new = _frames(False), _frames(True)
    for f, (a, b) in enumerate(zip(old, new)):
        for name, pa, pb in zip(PLANES, a, b):
            np.testing.assert_array_equal(pb.view(np.uint32), pa.view(np.uint32), err_msg="%s frame %d" % (name, f))
    assert old[1][0][..., :3].std() > 0.0


def test_terrain_ms():
    r = _renderer()
    with pytest.raises(vxpt.VxptError):
        r.terrain_ms()
    _ex(r, T.CASES[1])
    ms = r.terrain_ms()
    assert ms.shape == (4,) and np.isfinite(ms).all() and (ms >= 0.0).all() and ms.sum() > 0.0
    r.set_world_build("host")  # the host path has no kernels to time
    _ex(r, T.CASES[1])
    with pytest.raises(vxpt.VxptError):
        r.terrain_ms()
    r.close()


def test_bad_descriptors_leave_the_world_alone():
    r = _renderer()
    _ex(r, T.CASES[1])
    before = {n: r.read(n) for n in TABLES}
    for bad in (dict(origin=(0, 5, 0)), dict(origin=(1 << 24, 0, 0)), dict(freq_den=0.0), dict(chunks=(0, 1, 1))):
        with pytest.raises(vxpt.VxptError):
            r.generate_terrain(**dict(dict(chunks=(2, 1, 2), freq_den=64.0, ex=True), **bad))
    for n in TABLES:
        np.testing.assert_array_equal(r.read(n), before[n], err_msg=n)
    r.close()


def test_cli_terrain_seed_and_origin(tmp_path):
    """the executable's frame against the Python mirror of the same entry points (host world-build mode
    there, the device's here), replaying the executable's frame times as test_offline_cli does"""
    w, h, frames = 64, 48, 4
    prefix = str(tmp_path / "off")
    res = subprocess.run([EXE, "--width", str(w), "--height", str(h), "--frames", str(frames), "--output", prefix,
                          "--terrain-seed", "7", "--terrain-origin", "64,0,0", "--world-build", "device",
                          "--perf-report", str(tmp_path / "perf.txt")], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    rr = vxpt.Renderer(w, h)
    rr.load_settings()
    rr.generate_terrain((2, 1, 2), origin=(64, 0, 0), seed=7)
    np.testing.assert_array_equal(rr.read("VOXELS"), vxpt.terrain_host((2, 1, 2), origin=(64, 0, 0), seed=7))
    cam = rr.scene_camera(os.path.join(REPO, "data", "scene", "scene_export.yaml"))
    c = (list(cam.pos), list(cam.dir), cam.fov_deg)
    rr.set_camera(*c[:2], fov=c[2], prev=c)
    rr.set_sky()
    dp, pp = rr.denoise_params(), rr.post_params()
    rows = [ln.split(",") for ln in open(prefix + "_frames.csv") if ln[0].isdigit()]
    dts = [float(x[7]) for x in rows]
    assert len(dts) == frames
    for f in range(frames):
        rr.render_frame(f, 1, dp)
        rr.postprocess(pp, dts[f])
    mine = str(tmp_path / "py.png")
    rr.write_png(mine)
    # another seed and origin is another picture
    rr.generate_terrain((2, 1, 2))
    rr.render_frame(0, 1, dp)
    rr.postprocess(pp, dts[0])
    other = str(tmp_path / "other.png")
    rr.write_png(other)
    rr.close()
    a, b = vxpt.read_png(mine), vxpt.read_png("%s_%04d.png" % (prefix, frames - 1))
    np.testing.assert_array_equal(a, b)
    assert a.std() > 1.0 and not np.array_equal(a, vxpt.read_png(other))
    for bad in (("--terrain-origin", "1,2"), ("--terrain-seed", "x7"), ("--terrain-origin", "0,5,0")):
        res = subprocess.run([EXE, "--width", "64", "--height", "48", "--frames", "1", "--output", prefix, *bad],
                             cwd=REPO, capture_output=True, text=True, timeout=60)
        assert res.returncode != 0, bad
