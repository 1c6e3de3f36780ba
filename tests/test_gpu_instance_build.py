"""Instanced-block edits with no host wait (vxpt_set_instance_build): the device TLAS
(a linear BVH, csrc/instances.hip + lbvh.hpp) and the device light tables against the host twins and
against host mode, on the C1 world with the lanterns and leaves of tests/test_gpu_meshes.py at 64x36."""
import os

import numpy as np
import pytest

import alias_ref
import instance_scene as sc
import vxpt
from golden.make_golden import C1_CAMERA
from instance_scene import dense_world as _dense_world, world as _world
from test_gpu_brick_pass import BUFFERS
from test_gpu_meshes import BASE, CH, LEAVES, LIGHT, _idx
from test_gpu_parity import _dn_params
from test_lights import _base_obj, _random_mesh_obj

pytestmark = pytest.mark.gpu

W, H = 64, 36


@pytest.fixture(scope="module")
def terrain():
    ids = sc.terrain_ids()
    r = vxpt.Renderer(W, H)  # the library's generator makes the same world
    r.generate_terrain(CH)
    np.testing.assert_array_equal(r.read("VOXELS"), ids)
    r.close()
    return ids


@pytest.fixture(params=["reference", "synthetic"])
def models(tmp_path, request):
    return sc.write_models(str(tmp_path), request.param)


def _renderer(ids, models, mode, world_build="host", chunks=CH):
    r = vxpt.Renderer(W, H)
    r.load_settings()
    if world_build != "host":
        r.set_world_build(world_build)
    r.upload_voxels(ids, chunks)
    if mode != "host":
        r.set_instance_build(mode)  # before the models: applied at load_models
    assert r.load_models(models) >= 3
    cam = (C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2])
    r.set_camera(*cam[:2], fov=cam[2], prev=cam)
    r.set_sky(0.25, 45.0, 0.0, 1.0)
    return r


def _root_box(r, block):
    """The block's BLAS root box as build_bvh makes it: the triangles' bounds widened in float32."""
    pos, _ = r.model(block)
    lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
    e, one = np.float32(1e-4), np.float32(1.0)
    return lo - e * (one + np.abs(lo)), hi + e * (one + np.abs(hi))


def _expected_tlas(r):
    """vxpt.lbvh_host of the context's instance rows -> (nodes, MeshInst rows in leaf order)."""
    inst = r.instances()
    meshed = {b: len(r.model(b)[0]) > 0 for b in set((inst[:, 0] + 1).tolist())}
    rows = [(i, row) for i, row in enumerate(inst) if meshed[int(row[0]) + 1]]
    boxes = np.zeros((len(rows), 6), np.float32)
    keys = np.zeros(len(rows), np.uint64)
    mi = np.zeros(len(rows), vxpt.MESH_INST_DTYPE)
    roots = {}
    for m, (i, row) in enumerate(rows):
        block = int(row[0]) + 1
        lo, hi = roots.setdefault(block, _root_box(r, block))
        cell = row[2:5].astype(np.float32)
        boxes[m, :3], boxes[m, 3:] = lo + cell, hi + cell
        keys[m] = vxpt.lbvh_key(int(row[2]), int(row[3]), int(row[4]), int(row[0]))
        mi[m] = (cell, block, i)
    nodes, order = vxpt.lbvh_host(boxes, keys)
    return nodes, mi[order]


def _tables(r):
    mp, recs, bins, lum = r.lights()
    nodes, mi = r.tlas()
    return dict(instances=r.instances(), tlas=nodes, mesh_inst=mi, mapping=mp, lights=recs, alias=bins, lum=lum,
                weights=r.light_weights(), row_light=r.mesh_row_light())


def _same_tables(a, b, tag, skip=()):
    for k in a:
        if k in skip:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, k)


def _check_device_tables(r, tag):
    """Device-mode tables against the host twins: TLAS bits, alias table, luminance sum."""
    t = _tables(r)
    nodes, mi = _expected_tlas(r)
    assert t["tlas"].tobytes() == nodes.tobytes(), tag
    assert t["mesh_inst"].tobytes() == mi.tobytes(), tag
    if len(t["weights"]):
        q, p, a, s = vxpt.alias_build_host(t["weights"])
        assert t["alias"]["q"].tobytes() == q.tobytes() and t["alias"]["p"].tobytes() == p.tobytes(), tag
        np.testing.assert_array_equal(t["alias"]["alias"], a, err_msg=tag)
        assert np.float32(t["lum"]).tobytes() == np.float32(s).tobytes(), tag
        alias_ref.check_valid(t["alias"]["q"], t["alias"]["alias"], t["alias"]["p"])
        assert alias_ref.recon_error(t["alias"]["p"], t["alias"]["q"], t["alias"]["alias"]) < 1e-4, tag
    return t


def _lantern_sequence(placed):
    first, width = 13, CH[0] * 32
    key = lambda p: first + (LIGHT - 1) * width ** 3 + p[0] + width * (p[2] + width * p[1])
    lanterns = sorted((p for p in placed if p[3] == LIGHT), key=key)
    assert len(lanterns) >= 2
    leaves = [p for p in placed if p[3] == LEAVES]
    seq = [(lanterns[-1][:3], 0), (lanterns[0][:3], 0), (lanterns[-1][:3], LIGHT)]
    if leaves:
        seq.append((leaves[0][:3], 0))
    return seq


# ---- 1. TLAS bits ----
def test_tlas_equals_host_twin(terrain, models):
    ids, placed = _world(terrain)
    r = _renderer(ids, models, "device")
    try:
        n, m = r.mesh_instance_count()
        assert n == len(placed) + sum(1 for p in placed if p[3] == LIGHT) and m == 2 * n - 1
        _check_device_tables(r, "scene")
    finally:
        r.close()


@pytest.mark.parametrize("count", [1, 0])
def test_tlas_of_one_and_of_no_instance(terrain, models, count):
    ids, placed = _world(terrain, keep=(LEAVES,))
    for x, y, z, _ in placed[count:]:
        ids[_idx(x, y, z)] = 0
    r = _renderer(ids, models, "device")
    try:
        assert r.mesh_instance_count() == ((1, 1) if count else (0, 0))
        nodes, mi = r.tlas()
        exp_nodes, exp_mi = _expected_tlas(r)
        assert nodes.tobytes() == exp_nodes.tobytes() and mi.tobytes() == exp_mi.tobytes()
        if count:
            assert nodes[0]["count"] == 1 and nodes[0]["left"] == 0
        rays = sc.rays(256, 3)
        out, _ = r.mesh_probe(rays)
        assert count or not out[:, 3].any()
    finally:
        r.close()


# ---- 2. same hits ----
def test_same_hits_in_both_modes(terrain, models):
    ids = _dense_world(terrain)
    rays = sc.rays()  # the rays of tests/test_instance_hits_precheck.py, which checks the cap's condition
    res = {}
    for mode in ("host", "device"):
        r = _renderer(ids, models, mode)
        try:
            res[mode] = [r.mesh_probe(rays, cull=False), r.mesh_probe(rays, cull=True), r.mesh_occluded(rays)]
        finally:
            r.close()
    assert res["host"][0][0][:, 3].sum() > 200  # the rays do hit meshes
    for k in (0, 1):
        (oh, ih), (od, idv) = res["host"][k], res["device"][k]
        assert oh[:, 0].tobytes() == od[:, 0].tobytes() and oh[:, 3].tobytes() == od[:, 3].tobytes(), "t / hit flag"
        differ = (ih != idv).any(1) | (oh[:, 1:3] != od[:, 1:3]).any(1)
        print("cull %d: %d of %d rays hit another triangle at the same t" % (k, differ.sum(), len(rays)))
        assert differ.sum() <= 1e-3 * len(rays)
    np.testing.assert_array_equal(res["host"][2], res["device"][2])


# ---- 3. light tables ----
def test_light_tables_equal_host_mode(terrain, models):
    ids, _ = _world(terrain)
    h, d = _renderer(ids, models, "host"), _renderer(ids, models, "device")
    try:
        th, td = _tables(h), _check_device_tables(d, "lights")
        assert len(td["lights"]) > 0
        _same_tables(th, td, "host vs device", skip=("tlas", "mesh_inst", "alias", "lum"))
        assert (td["row_light"] >= 0).sum() == len(td["mapping"]) > 0  # meshRowLight: compared above, bit for bit
        np.testing.assert_allclose(td["lum"], th["lum"], rtol=1e-6)
    finally:
        h.close()
        d.close()


# ---- 4. incremental equals full ----
def test_edits_equal_a_fresh_build_and_host_remap(terrain, models):
    ids, placed = _world(terrain)
    d, h = _renderer(ids, models, "device"), _renderer(ids, models, "host")
    try:
        cur = ids.copy()
        for k, ((x, y, z), block) in enumerate(_lantern_sequence(placed)):
            d.set_block(x, y, z, block)
            h.set_block(x, y, z, block)
            cur[_idx(x, y, z)] = block
            np.testing.assert_array_equal(d.read("VOXELS"), cur)
            got = _check_device_tables(d, "edit %d" % k)
            f = _renderer(cur, models, "device")
            try:
                _same_tables(got, _tables(f), "edit %d vs fresh" % k)
            finally:
                f.close()
            (rd, pd), (rh, ph) = d.light_remap(), h.light_remap()
            assert pd == ph
            np.testing.assert_array_equal(rd, rh, err_msg="edit %d remap" % k)
            _same_tables(_tables(h), got, "edit %d vs host" % k, skip=("tlas", "mesh_inst", "alias", "lum"))
    finally:
        d.close()
        h.close()


def test_instance_set_follows_200_random_edits(models):
    """The kept instance set against host mode's scan of the edited grid after every edit, on a 64^3
    grid, and against a fresh context at the end; then a non-cubic world, which keeps the scan."""
    rng = np.random.default_rng(9)
    for chunks, edits in (((2, 2, 2), 200), ((1, 2, 1), 60)):
        dims = np.array([chunks[0] * 32, chunks[1] * 32, chunks[2] * 32])
        ids = np.zeros(int(np.prod(chunks)) * 32768, np.uint8)
        d, h = _renderer(ids, models, "device", chunks=chunks), _renderer(ids, models, "host", chunks=chunks)
        try:
            cells = rng.integers(0, np.minimum(dims, 6), (edits, 3)) * (dims // 6 - 1)  # few cells: many re-edits
            cells[::7] = dims - 1  # the clamped corner
            for (x, y, z), b in zip(cells, rng.choice([0, 0, LEAVES, BASE, LIGHT, 1, 13], edits)):
                d.set_block(int(x), int(y), int(z), int(b))
                h.set_block(int(x), int(y), int(z), int(b))
                np.testing.assert_array_equal(d.instances(), h.instances())
                np.testing.assert_array_equal(d.lights()[0], h.lights()[0])
            f = _renderer(d.read("VOXELS"), models, "device", chunks=chunks)
            try:
                _same_tables(_tables(d), _tables(f), "after the edits %s" % (chunks,))
            finally:
                f.close()
        finally:
            d.close()
            h.close()


# ---- 5. frames without emissive instances ----
@pytest.mark.parametrize("world_build", ["host", "device"])
def test_leaves_only_frames_are_host_modes(terrain, models, world_build):
    ids, placed = _world(terrain, keep=(LEAVES,))
    a, b = _renderer(ids, models, "host", world_build), _renderer(ids, models, "device", world_build)
    p = _dn_params()
    try:
        for f in range(3):
            if f == 2:
                for r in (a, b):
                    r.set_block(*placed[0][:3], 0)
            for r in (a, b):
                r.render_frame(f, 1, p)
            for name in BUFFERS:
                assert a.read(name).tobytes() == b.read(name).tobytes(), (f, name)
    finally:
        a.close()
        b.close()


# ---- 6. frames with lanterns ----
def _edit_frames(ids, models, seq, how):
    """3 frames with the edits between them; how: "single" set_block, "batch1" set_blocks of one."""
    r = _renderer(ids, models, "device")
    p = _dn_params()
    out = []
    try:
        for f in range(3):
            if f > 0:
                (x, y, z), b = seq[f - 1]
                if how == "single":
                    r.set_block(x, y, z, b)
                else:
                    r.set_blocks([(x, y, z)], [b])
            r.render_frame(f, 1, p)
            out.append({n: r.read(n).tobytes() for n in BUFFERS})
        return out, _tables(r)
    finally:
        r.close()


def test_lantern_frames_single_and_batched(terrain, models):
    ids, placed = _world(terrain)
    seq = _lantern_sequence(placed)
    a, ta = _edit_frames(ids, models, seq, "single")
    b, tb = _edit_frames(ids, models, seq, "batch1")
    for f in range(3):
        for n in BUFFERS:
            assert a[f][n] == b[f][n], (f, n)
    _same_tables(ta, tb, "single vs batch of one")
    # two edits as one batch: the frame after it and the final tables are the two singles'
    p = _dn_params()
    got = []
    for batch in (False, True):
        r = _renderer(ids, models, "device")
        try:
            r.render_frame(0, 1, p)
            if batch:
                r.set_blocks([seq[0][0], seq[1][0]], [seq[0][1], seq[1][1]])
            else:
                r.set_block(*seq[0][0], seq[0][1])
                r.set_block(*seq[1][0], seq[1][1])
            r.render_frame(1, 1, p)
            got.append(({n: r.read(n).tobytes() for n in BUFFERS}, _tables(r), r.light_remap()))
        finally:
            r.close()
    for n in BUFFERS:
        assert got[0][0][n] == got[1][0][n], ("batch of two", n)
    _same_tables(got[0][1], got[1][1], "batch of two")
    np.testing.assert_array_equal(got[0][2][0], got[1][2][0])


def _uneven_light_obj(path):
    """An emissive mesh whose triangles differ in area by up to 12x, so that the light weights are
    unequal and the alias table's pairing matters."""
    with open(path, "w") as f:
        f.write("vt 0 0\n")
        k = 0
        for i, w in enumerate((0.04, 0.08, 0.16, 0.3, 0.48)):
            y = 0.1 + 0.1 * i
            for v in ((0.26, y, 0.3), (0.26 + w, y, 0.3), (0.26, y + 0.08, 0.3 + w)):
                f.write("v %g %g %g\n" % v)
            f.write("f %d/1 %d/1 %d/1\n" % (k + 1, k + 2, k + 3))
            k += 3


def test_lantern_frame_means_agree_between_modes(terrain, tmp_path):
    """Frame 2's radiance at 16 spp in host and in device mode, with a light mesh of unequal triangles:
    the device table is another valid alias table of the same weights than Vose's (asserted), so the
    frame draws other light samples.  The mean over the pixels that see no sky agrees within 3 x the
    spread between two host-mode renders of the same frame at frame_num and frame_num + 1000.
    Measured figures: DESIGN.md §9.5."""
    models = sc.write_models(str(tmp_path), "synthetic")
    _uneven_light_obj(os.path.join(models, "models", sc.MODEL_FILES[LIGHT]))
    ids, placed = _world(terrain)
    seq = _lantern_sequence(placed)
    p = _dn_params()

    def frame(mode, frame_num, spp=16):
        r = _renderer(ids, models, mode)
        try:
            for f in range(2):
                if f > 0:
                    r.set_block(*seq[0][0], seq[0][1])
                r.render_frame(f, 1, p)
            r.set_block(*seq[1][0], seq[1][1])
            t = _tables(r)
            r.render_frame(frame_num, spp, p)
            ill, depth = r.read("ILLUM")[..., :3].astype(np.float64), r.read("DEPTH")
            return ill[depth < 1e26].mean(), t
        finally:
            r.close()

    (h0, th), (h1, _), (d0, td) = frame("host", 2), frame("host", 1002), frame("device", 2)
    assert len(th["weights"]) > 0 and th["weights"].tobytes() == td["weights"].tobytes()
    assert len(set(th["weights"].tolist())) > 1
    assert th["alias"].tobytes() != td["alias"].tobytes(), "the two constructions pair the same bins here"
    spread = abs(h0 - h1)
    print("host mean %.6g, host spread %.3g (%.2f %%), device - host %.3g" % (h0, spread, 100 * spread / h0, d0 - h0))
    assert spread <= 0.05 * h0
    assert abs(d0 - h0) <= 3 * spread


# ---- 7. coalescing and waits ----
def test_batches_coalesce_and_do_not_wait(terrain, models):
    ids, _ = _world(terrain)
    free = [(x, 31, 20) for x in range(64) if ids[_idx(x, 31, 20)] == 0][:8]
    assert len(free) == 8
    for mode, batch, exp in (("device", True, (1, 1, 1, 0)), ("device", False, (8, 8, 8, 0)), ("host", False, None)):
        r = _renderer(ids, models, mode)
        try:
            s0 = r.instance_build_stats().astype(np.int64)
            if batch:
                r.set_blocks(free, [LIGHT] * 8)
            else:
                for c in free:
                    r.set_block(*c, LIGHT)
            s = r.instance_build_stats().astype(np.int64) - s0
            if exp:
                assert tuple(s) == exp, (mode, batch, s)
            else:
                assert s[0] == 8 and s[3] >= 8, s
            assert len(r.lights()[0]) == len(_renderer_lights(ids, models)) + 8
        finally:
            r.close()


def _renderer_lights(ids, models):
    r = _renderer(ids, models, "host")
    try:
        return r.lights()[0]
    finally:
        r.close()


# ---- 8. mode switch ----
def test_mode_switch_rebuilds_and_returns_to_host_bits(terrain, models):
    ids, _ = _world(terrain)
    a, b = _renderer(ids, models, "host"), _renderer(ids, models, "host")
    p = _dn_params()
    try:
        host_tables = _tables(b)
        b.set_instance_build("device")
        _check_device_tables(b, "switched to device")
        b.set_instance_build("host")
        _same_tables(host_tables, _tables(b), "back in host mode")
        for f in range(2):
            a.render_frame(f, 1, p)
            b.render_frame(f, 1, p)
            for n in BUFFERS:
                assert a.read(n).tobytes() == b.read(n).tobytes(), (f, n)
    finally:
        a.close()
        b.close()


# ---- 9. refusals ----
def test_bad_mode_is_refused_and_early_mode_is_kept(terrain, models):
    ids, _ = _world(terrain)
    r = vxpt.Renderer(W, H)
    try:
        assert r.lib.vxpt_set_instance_build(r.ctx, 2) == -1  # VXPT_ERR_ARG
        assert r.lib.vxpt_set_instance_build(r.ctx, -1) == -1
        with pytest.raises(vxpt.VxptError):
            r.set_instance_build("gpu")
        r.load_settings()
        r.set_instance_build("device")  # no world, no models yet
        assert tuple(r.instance_build_stats()) == (0, 0, 0, 0)
        r.upload_voxels(ids, CH)
        assert r.load_models(models) >= 3
        assert r.instance_build_stats()[0] == 1
        _check_device_tables(r, "mode set before the models")
    finally:
        r.close()
