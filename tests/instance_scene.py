"""The scenes and rays shared by tests/test_gpu_instance_build.py (GPU) and
tests/test_instance_hits_precheck.py (CPU): the C1 terrain from the oracle's CPU generator, the
lanterns and leaves of tests/test_gpu_meshes.py on it, and seeded random rays through its bounds."""
import os
import shutil

import numpy as np

import oracle
from test_gpu_meshes import BASE, CH, GOLDEN_MODELS, LEAVES, LIGHT, _idx, place_meshes
from test_lights import _base_obj, _prism_obj, _random_mesh_obj

RAY_SEED, N_RAYS = 11, 20000
MODEL_FILES = {LIGHT: "lanternLight.obj", BASE: "lanternBase.obj", LEAVES: "leavesCube4.obj"}


def terrain_ids():
    o = oracle.Oracle(8, 8)
    o.terrain(CH)
    ids = np.array(o.voxels(), np.uint8).reshape(-1).copy()
    ids.setflags(write=False)
    return ids


def write_models(root, kind):
    """<root>/models/*.obj: the reference's meshes (tests/golden/models) or the synthetic ones."""
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    path = lambda f: os.path.join(root, "models", f)
    if kind == "reference":
        for f in MODEL_FILES.values():
            shutil.copy(os.path.join(GOLDEN_MODELS, f), path(f))
    else:
        _prism_obj(path(MODEL_FILES[LIGHT]))
        _base_obj(path(MODEL_FILES[BASE]))
        _random_mesh_obj(path(MODEL_FILES[LEAVES]), n=120)
    return root


def world(terrain, keep=(LIGHT, LEAVES)):
    ids = terrain.copy()
    placed = place_meshes(ids)
    for x, y, z, b in placed:
        if b not in keep:
            ids[_idx(x, y, z)] = 0
    return ids, [p for p in placed if p[3] in keep]


def dense_world(terrain):
    """The C1 scene plus leaves and lanterns scattered in the air, so that random rays hit meshes."""
    ids, _ = world(terrain)
    rng = np.random.default_rng(5)
    for x, y, z in rng.integers((8, 20, 8), (56, 31, 56), (400, 3)):
        if ids[_idx(int(x), int(y), int(z))] == 0:
            ids[_idx(int(x), int(y), int(z))] = (LEAVES, LIGHT, BASE)[int(x + y + z) % 3]
    return ids


def rays(n=N_RAYS, seed=RAY_SEED):
    rng = np.random.default_rng(seed)
    lo, hi = np.zeros(3), np.array([CH[0] * 32, CH[1] * 32, CH[2] * 32], np.float64)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((n, 8), np.float32)
    out[:, :3], out[:, 3], out[:, 4:7], out[:, 7] = o, 1e-3, d, 1e30
    return out
