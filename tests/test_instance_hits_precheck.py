"""The condition behind tests/test_gpu_instance_build.py::test_same_hits_in_both_modes, checked on the
CPU: on the test's scene and rays, the host BVH over the instances in their order against the same
instances permuted (tests/native/mesh_walk_driver.hip, the library's own builder and walk).  Another
tree may find another triangle at the same distance; such rays must stay within 1e-3 of the rays with
the reference alone, or the cap the GPU test puts on host against device mode means nothing.  If this
fails, change instance_scene.RAY_SEED, not the cap.  No GPU."""
import subprocess

import numpy as np
import pytest

import instance_scene as sc
import oracle
from test_lights import BLOCKS, mesh_walk_driver  # noqa: F401  (the fixture that compiles the driver)


def _run(driver, tmp, name, models, rows, rays):
    with open(tmp / (name + ".bin"), "wb") as f:
        for b in range(32):
            t = np.asarray(models.get(b, np.zeros((0, 3, 3))), np.float32).reshape(-1, 9)
            f.write(np.int32(len(t)).tobytes())
            f.write(t.tobytes())
        f.write(np.int32(len(rows)).tobytes())
        f.write(np.ascontiguousarray(rows, np.int32).tobytes())
    res = subprocess.run([driver, str(tmp / (name + ".bin")), str(tmp / "rays.bin"), str(tmp / (name + ".out"))],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return np.fromfile(tmp / (name + ".out"), np.int32).reshape(-1, 13)


@pytest.mark.parametrize("kind", ["reference", "synthetic"])
def test_reference_alone_stays_within_the_cap(mesh_walk_driver, tmp_path, kind):  # noqa: F811
    ids = sc.dense_world(sc.terrain_ids())
    rows = oracle.collect_instances(ids, sc.CH, BLOCKS)
    sc.write_models(str(tmp_path), kind)
    models = {b: oracle.parse_obj(str(tmp_path / "models" / f))[0] for b, f in sc.MODEL_FILES.items()}
    rays = sc.rays()
    rays.tofile(tmp_path / "rays.bin")
    perm = np.random.default_rng(3).permutation(len(rows))
    a = _run(mesh_walk_driver, tmp_path, "ordered", models, rows, rays)
    b = _run(mesh_walk_driver, tmp_path, "permuted", models, rows[perm], rays)
    assert a[:, 3].sum() > 200  # the rays do hit meshes
    for cull in (0, 1):
        x, y = a[:, 6 * cull:6 * cull + 6].copy(), b[:, 6 * cull:6 * cull + 6].copy()
        hit = y[:, 3] == 1
        y[hit, 4] = perm[y[hit, 4]]  # a row of the permuted list -> the row of the ordered one
        np.testing.assert_array_equal(x[:, 0], y[:, 0], err_msg="t")
        np.testing.assert_array_equal(x[:, 3], y[:, 3], err_msg="hit flag")
        differ = (x[:, [1, 2, 4, 5]] != y[:, [1, 2, 4, 5]]).any(1)
        print("cull %d: %d of %d rays find another triangle at the same t" % (cull, differ.sum(), len(rays)))
        assert differ.sum() <= 1e-3 * len(rays)
    np.testing.assert_array_equal(a[:, 12], b[:, 12], err_msg="occluded")
