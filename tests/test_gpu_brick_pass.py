"""vxpt_tuning.brick_pass (the walk crosses an occupied brick with no cube in the ray's octant like
an empty box: vx_device.hpp brick_passes) changes no result: frames with brick_pass = 0 (every
occupied brick walked cell by cell) equal the default's bit for bit, every output and state buffer.
The C1 scene at 256 x 144, and a 64^3 world with world-y heights (64 of 128 levels of terrain: rays
leave it through the world's sides and top).  The mesh kernels walk the BVH, not the voxel grid, and
do not take the switch, so no mesh frame is added here.
"""
import numpy as np
import pytest

import vxpt
from golden.make_golden import C1_CAMERA
from test_gpu_parity import _dn_params

BUFFERS = ("ILLUM", "DEPTH", "NORMAL_ROUGH", "GEO_NORMAL_THIN", "ALBEDO", "MATERIAL", "MAT_PARAM", "MOTION",
           "TAP_RECORD", "RES_EVEN", "RES_ODD", "PREV_ILLUM", "PREV_FAST", "HIST_LEN", "PREV_HIST_LEN", "PREV_DEPTH",
           "OUTPUT")


def _renderer(world, brick_pass):
    r = vxpt.Renderer(256, 144)
    r.load_settings()
    pos, d, fov = C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2]
    if world == "c1":
        r.generate_terrain((2, 1, 2), height_scale=32.0)
    else:
        r.generate_terrain((2, 2, 2), height_scale=64.0, freq_den=64.0, global_y=True)
        pos = (pos[0], pos[1] * 2.0, pos[2])
    r.set_camera(pos, d, fov=fov, prev=(pos, d, fov))
    r.set_sky(0.25, 45.0, 0.0, 1.0)
    assert r.tuning()["brick_pass"] == 1  # the default
    r.set_tuning(brick_pass=brick_pass)
    assert r.tuning()["brick_pass"] == brick_pass
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("world", ["c1", "y64"])
def test_brick_pass_changes_no_result(world):
    a, b = _renderer(world, 1), _renderer(world, 0)
    p = _dn_params()
    try:
        a.render_frames(0, 2, 2, p)
        b.render_frames(0, 2, 2, p)
        for name in BUFFERS:
            x, y = a.read(name), b.read(name)
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=name)
        assert np.isfinite(a.read("OUTPUT")).all() and a.read("DEPTH").min() < 5e5  # terrain in view
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_brick_pass_out_of_range_is_refused():
    r = vxpt.Renderer(64, 48)
    try:
        with pytest.raises(vxpt.VxptError):
            r.set_tuning(brick_pass=2)
        assert r.tuning()["brick_pass"] == 1
    finally:
        r.close()
