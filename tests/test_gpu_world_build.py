"""The world's tables built and edited on the device (vxpt_set_world_build, csrc/world.hip) against the
host build, which stays the default and the yardstick: integer tables, so everything is bit-equal.

Builds: device mode against host mode and against vxpt.world_tables_host, with and without the box
tables and with other caps.  Edits: test_edits' 400 random edits, its emptied brick and lone cube, plus
a cell edited twice in one batch and a cube on the world's top row, one by one and in batches of 1, 7
and 64, against a host-mode full rebuild of the edited grid and the oracle's DDA on it.

The sky-exit table after edits is compared with a host-mode renderer given the same edits, not with the
full rebuild: an edit raises a column top and never lowers it (a bound, in both modes), so once an edit
removes a column's highest cube the edited table stays above the rebuilt one.  The test checks that
bound as well.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle
import vxpt
from golden.make_golden import C1_CAMERA
from test_edits import CH, EXE, REPO, STRUCTS, _idx, _mirror, _random_edits
from test_oracle import _random_rays

pytestmark = pytest.mark.gpu

TABLES = STRUCTS + ("SKY_TOP",)
PLANES = ("OUTPUT", "ILLUM", "DEPTH", "NORMAL_ROUGH", "GEO_NORMAL_THIN", "ALBEDO", "MATERIAL", "MAT_PARAM", "MOTION")


def _renderer(mode, boxes=1, caps=(32, 32)):
    r = vxpt.Renderer(64, 64)
    r.load_settings()
    r.set_tuning(dda_boxes=boxes, box_cap=caps[0], box_cap_up=caps[1])
    r.set_world_build(mode)
    return r


def _names(boxes=1):
    return tuple(n for n in TABLES if boxes or n != "BOX_TABLES")


def _assert_same(a, b, names=TABLES):
    for name in names:
        np.testing.assert_array_equal(a.read(name), b.read(name), err_msg=name)


_WORLD_CACHE = {}


def _world(kind, chunks):
    if (kind, chunks) not in _WORLD_CACHE:
        n = int(np.prod(chunks)) * 32768
        if kind == "terrain":
            r = vxpt.Renderer(64, 64)
            r.generate_terrain(chunks)
            ids = r.read("VOXELS").copy()
            r.close()
        elif kind == "random":
            rng = np.random.default_rng(3)
            ids = np.where(rng.random(n) < 0.03, rng.choice(np.array([0, 1, 7, 12, 13, 16, 29], np.uint8), n), 0)
            ids = ids.astype(np.uint8)
        else:
            ids = np.zeros(n, np.uint8)
        _WORLD_CACHE[kind, chunks] = ids
    return _WORLD_CACHE[kind, chunks]


@pytest.mark.parametrize("boxes,caps", [(1, (32, 32)), (1, (8, 16)), (0, (32, 32))])
@pytest.mark.parametrize("chunks", [(2, 1, 2), (1, 2, 3)])
@pytest.mark.parametrize("kind", ["terrain", "random", "empty"])
def test_device_build_equals_host_build_and_host_twin(kind, chunks, boxes, caps):
    ids = _world(kind, chunks)
    h, d = _renderer("host", boxes, caps), _renderer("device", boxes, caps)
    h.upload_voxels(ids, chunks)
    d.upload_voxels(ids, chunks)
    _assert_same(d, h, _names(boxes))
    twin = vxpt.world_tables_host(ids, chunks, *caps)
    for name in _names(boxes):
        if name != "VOXELS":
            np.testing.assert_array_equal(d.read(name), twin[name], err_msg=name)
    h.close()
    d.close()


def test_generate_terrain_in_device_mode():
    h, d = _renderer("host"), _renderer("device")
    h.generate_terrain(CH)
    d.generate_terrain(CH)
    _assert_same(d, h)
    h.close()
    d.close()


def test_tuning_changes_in_device_mode():
    ids = _world("terrain", CH)
    d = _renderer("device", boxes=0)
    d.upload_voxels(ids, CH)
    for boxes, caps in ((1, (8, 16)), (1, (32, 32)), (0, (32, 32)), (1, (1, 255))):
        d.set_tuning(dda_boxes=boxes, box_cap=caps[0], box_cap_up=caps[1])
        h = _renderer("host", boxes, caps)
        h.upload_voxels(ids, CH)
        _assert_same(d, h, _names(boxes))
        h.close()
    d.close()


def test_mode_switches_with_a_world_loaded():
    ids = _world("random", (1, 2, 3))
    h = _renderer("host")
    h.upload_voxels(ids, (1, 2, 3))
    r = _renderer("host")
    r.upload_voxels(ids, (1, 2, 3))
    for mode in ("device", "host", "device"):
        r.set_world_build(mode)
        _assert_same(r, h)
    with pytest.raises(vxpt.VxptError):
        r.set_world_build("gpu")
    assert r.lib.vxpt_set_world_build(r.ctx, 2) == -1
    _assert_same(r, h)
    h.close()
    r.close()


class _Recorder:
    """stands in for a renderer in test_edits._random_edits: keeps the edits"""

    def __init__(self):
        self.edits = []

    def set_block(self, x, y, z, b):
        self.edits.append((x, y, z, b))


_EDITS = {}


def _edit_script():
    """(edits, edited ids, host-mode renderer after a full rebuild of them, host-mode renderer given the
    edits one by one, the oracle's answers for the probe rays): made once, only read afterwards"""
    if not _EDITS:
        ids = _world("terrain", CH).copy()
        rec = _Recorder()
        _random_edits(rec, ids, 400, 5)
        extra = [(21, 9, 33, 3), (21, 9, 33, 0),  # one cell twice: adjacent, so one batch holds both (sizes 7, 64)
                 (5, 31, 5, 3),                   # the world's top row: above every cube
                 (50, 2, 50, 16), (50, 2, 50, 4)]
        for x, y, z, b in extra:
            ids[_idx(x, y, z)] = b
        edits = rec.edits[:200] + extra + rec.edits[200:]
        for x, y, z, b in rec.edits[200:]:  # the script's order decides the final grid
            ids[_idx(x, y, z)] = b
        rebuilt = _renderer("host")
        rebuilt.upload_voxels(ids, CH)
        singles = _renderer("host")
        singles.upload_voxels(_world("terrain", CH), CH)
        for e in edits:
            singles.set_block(*e)
        np.testing.assert_array_equal(singles.read("VOXELS"), ids)
        o = oracle.Oracle(64, 64)
        o.set_voxels(ids, CH)
        probes = []
        for outside in (False, True):
            rays = _random_rays(4000, 31 + outside, outside=outside)
            probes.append((rays, o.rays(rays, 0), o.rays(rays, 2)))
        _EDITS.update(edits=edits, ids=ids, rebuilt=rebuilt, singles=singles, probes=probes)
    return _EDITS


@pytest.mark.parametrize("batch", [0, 1, 7, 64])
def test_device_edits_equal_full_rebuild_and_oracle_dda(batch):
    s = _edit_script()
    d = _renderer("device")
    d.upload_voxels(_world("terrain", CH), CH)
    edits = np.asarray(s["edits"], np.int32)
    if batch == 0:
        for e in s["edits"]:
            d.set_block(*e)
    else:
        for k in range(0, len(edits), batch):
            d.set_blocks(edits[k:k + batch, :3], edits[k:k + batch, 3])
    _assert_same(d, s["rebuilt"], STRUCTS)
    np.testing.assert_array_equal(d.read("SKY_TOP"), s["singles"].read("SKY_TOP"))
    assert (d.read("SKY_TOP") >= s["rebuilt"].read("SKY_TOP")).all()
    for rays, (c0, t0), (c2, _) in s["probes"]:
        g, tg = d.probe_rays(rays, 0)
        np.testing.assert_array_equal(g, c0)
        np.testing.assert_array_equal(tg.view(np.uint32), t0.view(np.uint32))
        occ, _ = d.probe_rays(rays, 2)
        np.testing.assert_array_equal(occ[:, 0], c2[:, 0])
    d.close()


def _light_state(r):
    mapping, records, alias, lum = r.lights()
    remap, pending = r.light_remap()
    return dict(mapping=mapping, records=records, alias=alias, lum=np.float32(lum), remap=remap,
                pending=np.array(pending), instances=r.instances())


@pytest.mark.parametrize("mode", ["host", "device"])
def test_set_blocks_equals_set_block(mode):
    """lanterns (16), their bases (15) and leaves (14) come and go inside the batches"""
    rng = np.random.default_rng(11)
    edits = []
    for _ in range(90):
        x, y, z = int(rng.integers(8, 24)), int(rng.integers(20, 30)), int(rng.integers(8, 24))
        edits.append((x, y, z, int(rng.choice([0, 0, 16, 16, 15, 14, 3]))))
    edits += [(10, 28, 10, 16), (11, 28, 10, 16), (10, 28, 10, 0), (12, 28, 12, 16)]
    edits = np.asarray(edits, np.int32)
    a, b = _renderer(mode), _renderer("host")
    for r in (a, b):
        r.upload_voxels(_world("terrain", CH), CH)
        assert r.load_models(os.path.join(REPO, "tests", "golden")) >= 3
    for k in range(0, len(edits), 13):
        a.set_blocks(edits[k:k + 13, :3], edits[k:k + 13, 3])
        for e in edits[k:k + 13]:
            b.set_block(*(int(v) for v in e))
        sa, sb = _light_state(a), _light_state(b)
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg="%s after edit %d" % (key, k))
    assert len(_light_state(a)["records"]) > 0
    _assert_same(a, b, STRUCTS)
    a.close()
    b.close()


def _frames(mode, spp):
    """frame 0, an edit of the block under the crosshair, frame 1 at once; then another edit and two
    frames through render_frames.  The planes after each step."""
    r = _renderer(mode)
    r.generate_terrain(CH)
    r.set_camera(C1_CAMERA[0], C1_CAMERA[1], fov=C1_CAMERA[2], prev=C1_CAMERA)
    r.set_sky()
    dp = r.denoise_params()
    out = []
    r.render_frame(0, spp, dp)
    out.append([r.read(n) for n in PLANES])
    pk = r.pick_block()
    assert pk["hit"]
    r.set_block(*pk["hit_pos"], 0)
    r.render_frame(1, spp, dp)
    out.append([r.read(n) for n in PLANES])
    pk = r.pick_block()
    assert pk["hit"] and pk["space"]
    r.set_blocks([pk["place_pos"], pk["hit_pos"]], [9, 0])
    r.render_frames(2, 2, spp, dp)
    out.append([r.read(n) for n in PLANES])
    r.close()
    return out


@pytest.mark.parametrize("spp", [1, 4])
def test_frames_around_an_edit_equal_host_mode(spp):
    host, dev = _frames("host", spp), _frames("device", spp)
    for step, (hs, ds) in enumerate(zip(host, dev)):
        for name, hp, dp in zip(PLANES, hs, ds):
            np.testing.assert_array_equal(dp.view(np.uint32), hp.view(np.uint32), err_msg="%s step %d" % (name, step))
    assert not np.array_equal(host[0][0], host[1][0])  # the edit is in view


@pytest.mark.parametrize("mode", ["host", "device"])
def test_a_bad_edit_refuses_the_whole_batch(mode):
    r = _renderer(mode)
    r.upload_voxels(_world("terrain", CH), CH)
    before = {n: r.read(n) for n in TABLES}
    for bad in ((64, 3, 3, 1), (3, -1, 3, 1), (3, 3, 3, 256)):
        e = np.asarray([(3, 3, 3, 0), (40, 30, 9, 5), bad, (4, 4, 4, 2)], np.int32)
        assert r.lib.vxpt_set_blocks(r.ctx, e.ctypes.data, len(e)) == -1
        with pytest.raises(vxpt.VxptError):
            r.set_blocks(e[:, :3], e[:, 3])
    for n in TABLES:
        np.testing.assert_array_equal(r.read(n), before[n], err_msg=n)
    r.set_blocks(np.zeros((0, 3), np.int32), np.zeros(0, np.int32))  # an empty batch is fine
    r.close()


def test_cli_world_build_device_writes_the_host_frames(tmp_path):
    """The scripted removals in device mode against the same run in host mode.  Two runs of the
    executable differ by their frame times (they drive the exposure adaptation), so the host-mode run is
    test_edits' Python mirror replaying the device run's frame times: the same entry points, host mode."""
    prefix = str(tmp_path / "dev")
    res = subprocess.run([EXE, "--width", "64", "--height", "64", "--frames", "16", "--output", prefix,
                          "--test-remove20", "--world-build", "device", "--perf-report", str(tmp_path / "perf.txt")],
                         cwd=REPO, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert res.stdout.count("EDIT: frame") >= 10
    rows = [ln.split(",") for ln in open(prefix + "_frames.csv") if ln[0].isdigit()]
    dts = [float(x[7]) for x in rows]
    out, _ = _mirror("remove20", 64, 64, 16, dts, {})
    mine = str(tmp_path / "host.png")
    vxpt.write_png(mine, out)
    assert open(mine, "rb").read() == open(prefix + "_0015.png", "rb").read()
    res = subprocess.run([EXE, "--world-build", "gpu"], cwd=REPO, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0
