"""vxpt_offline's --instance-build and --load-world (csrc/vxpt_offline.cpp).

CPU: the flags are listed and a bad or incomplete value is refused.
GPU: --instance-build device with --test-remove20 on the mesh scene writes its frames, and a saved edited
world with lanterns loaded through --load-world gives the first frame of the in-process world, in both
instance modes.
"""
import os

import numpy as np
import pytest

import instance_scene as sc
import vxpt
from golden.make_golden import C1_CAMERA
from test_gpu_meshes import CH, LIGHT
from test_offline_cli import run


def test_help_lists_the_flags_and_bad_values_are_refused():
    r = run("--help")
    assert r.returncode == 0 and "--instance-build" in r.stdout and "--load-world" in r.stdout
    assert run("--instance-build", "gpu").returncode == 2
    assert run("--load-world", "only_one_value").returncode == 2


def _saved_mesh_world(tmp_path, mode="host"):
    """The C1 mesh scene saved as a world file (camera: C1) -> (yaml, chunk dir, lanterns and leaves)."""
    sc.write_models(str(tmp_path), "reference")
    ids, placed = sc.world(sc.terrain_ids())
    r = vxpt.Renderer(64, 36)
    r.load_settings()
    r.upload_voxels(ids, CH)
    cam = (C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2])
    r.set_camera(*cam[:2], fov=cam[2], prev=cam)
    yaml_path, chunk_dir = str(tmp_path / "scene.yaml"), str(tmp_path / "scene_chunks")
    r.save_world(yaml_path, chunk_dir)
    r.close()
    return yaml_path, chunk_dir, placed


@pytest.mark.gpu
def test_remove20_in_device_mode_writes_its_frames(tmp_path):
    yaml_path, chunk_dir, _ = _saved_mesh_world(tmp_path)
    prefix = str(tmp_path / "off")
    r = run("--width", "64", "--height", "36", "--frames", "4", "--output", prefix, "--test-remove20",
            "--load-world", yaml_path, chunk_dir, "--instance-build", "device", "--world-build", "device",
            "--models", str(tmp_path), "--no-textures", "--perf-report", str(tmp_path / "perf.txt"), timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Instanced meshes loaded: 3" in r.stdout and "World loaded" in r.stdout
    for f in (0, 3):
        assert os.path.exists("%s_%04d.png" % (prefix, f))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "device"])
def test_load_world_round_trip(tmp_path, mode):
    w, h = 64, 36
    sc.write_models(str(tmp_path), "reference")
    ids, placed = sc.world(sc.terrain_ids())
    cam = (C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2])

    def renderer():
        r = vxpt.Renderer(w, h)
        r.load_settings()
        r.set_instance_build(mode)
        return r

    a = renderer()
    a.upload_voxels(ids, CH)
    assert a.load_models(str(tmp_path)) >= 3
    lantern = next(p for p in placed if p[3] == LIGHT)
    a.set_block(*lantern[:3], 0)  # an edited world: one lantern gone, another placed
    a.set_block(lantern[0] + 1, lantern[1], lantern[2], LIGHT)
    a.set_camera(*cam[:2], fov=cam[2], prev=cam)
    yaml_path, chunk_dir = str(tmp_path / "world.yaml"), str(tmp_path / "chunks")
    a.save_world(yaml_path, chunk_dir)
    edited = a.read("VOXELS").copy()
    a.close()

    prefix = str(tmp_path / "cli")
    r = run("--width", str(w), "--height", str(h), "--frames", "1", "--output", prefix, "--load-world", yaml_path,
            chunk_dir, "--instance-build", mode, "--models", str(tmp_path), "--no-textures",
            "--perf-report", str(tmp_path / "perf.txt"), timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "World loaded" in r.stdout

    # the in-process world: the edited grid, the saved camera, the CLI's frame time for the exposure
    b = renderer()
    b.upload_voxels(edited, CH)
    assert b.load_models(str(tmp_path)) >= 3
    c = b.scene_camera(yaml_path)
    c = (list(c.pos), list(c.dir), c.fov_deg)
    b.set_camera(*c[:2], fov=c[2], prev=c)
    b.set_sky()
    rows = [ln.split(",") for ln in open(prefix + "_frames.csv") if ln[0].isdigit()]
    b.render_frame(0, 1, b.denoise_params())
    b.postprocess(b.post_params(), float(rows[0][7]))
    mine = str(tmp_path / "py.png")
    b.write_png(mine)
    b.close()
    x, y = vxpt.read_png(mine), vxpt.read_png(prefix + "_0000.png")
    np.testing.assert_array_equal(x, y)
    assert x.std() > 1.0
