"""Render scale on the GPU: vxpt_upscale (csrc/upscale.hip) against vxpt_upscale_host, which runs
the same per-pixel bodies on the host.  The bar is bit equality: both sides are built without
contraction and with IEEE division and square root."""
import numpy as np
import pytest

import upscale_ref as ref
import vxpt
from upscale_ref import MODES, SHAPES

pytestmark = pytest.mark.gpu

# several 64x16 output tiles in both axes with ragged last tiles
TILED = ((70, 45), (131, 83))
MODE_NAMES = {0: "bicubic", 1: "easu", 2: "easu-sharp"}


def _image(w, h):
    img = ref.noise_image(w, h, seed=w * 1000 + h)
    img[h // 3: h // 3 + 2, : w // 2] = ref.smooth_image(w, h)[h // 3: h // 3 + 2, : w // 2]
    img[0, 0, :3] = 0.0  # a flat corner: the clamped taps of the corner outputs all read one value
    return img


def _assert_bits(got, want, what):
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), "%s: %d of %d values differ, max abs %.3e" % (
        what, diff.sum(), diff.size, np.abs(got.astype(np.float64) - want).max())


@pytest.mark.parametrize("shape", list(SHAPES) + [TILED], ids=["%dx%d-%dx%d" % (a + b) for a, b in list(SHAPES) + [TILED]])
def test_gpu_is_bit_equal_to_host(shape):
    (w, h), (ow, oh) = shape
    img = _image(w, h)
    r = vxpt.Renderer(w, h)
    try:
        r.write("FRAME", img)
        for mode in MODES:
            for sharp in ((1.0, 0.4) if mode == ref.EASU_SHARPEN else (1.0,)):
                got = r.upscale(ow, oh, mode, sharp)
                assert got.shape == (oh, ow, 4)
                _assert_bits(got, vxpt.upscale_host(img, ow, oh, mode, sharp), "%s %.1f" % (MODE_NAMES[mode], sharp))
        np.testing.assert_array_equal(r.read("FRAME"), img)
    finally:
        r.close()


def test_gpu_buffer_grows_and_shrinks():
    w, h = 24, 16
    img = _image(w, h)
    r = vxpt.Renderer(w, h)
    try:
        r.write("FRAME", img)
        for ow, oh in ((48, 32), (96, 80), (30, 20), (96, 80)):
            got = r.upscale(ow, oh, ref.EASU_SHARPEN, 1.0)
            assert r.upscale_info()[:2] == (ow, oh)
            _assert_bits(got, vxpt.upscale_host(img, ow, oh, ref.EASU_SHARPEN, 1.0), "%dx%d" % (ow, oh))
        for bad in ((w - 1, h), (w, h - 1)):
            with pytest.raises(vxpt.VxptError):
                r.upscale(*bad)
        with pytest.raises(vxpt.VxptError):
            r.upscale(48, 32, mode=3)
        with pytest.raises(vxpt.VxptError):
            r.upscale(48, 32, sharpness=1.5)
    finally:
        r.close()


def test_gpu_upscale_needs_a_frame():
    r = vxpt.Renderer(16, 16)
    try:
        with pytest.raises(vxpt.VxptError):
            r.upscale(32, 32)
    finally:
        r.close()


def test_gpu_rendered_frame_end_to_end():
    """The smoke scene at 64x48: render, post-process, upscale to 128x96 with the sharpener."""
    from golden.make_golden import C1_CAMERA

    w, h, ow, oh = 64, 48, 128, 96
    r = vxpt.Renderer(w, h)
    try:
        r.load_settings()
        r.generate_terrain((2, 1, 2))
        r.set_camera(C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2], prev=C1_CAMERA)
        r.set_sky()
        r.render_frame(0, 1, r.denoise_params())
        r.postprocess(r.post_params(), 16.6667)
        frame, output = r.read("FRAME"), r.read("OUTPUT")
        assert frame[..., :3].std() > 0.01  # a real image
        got = r.upscale(ow, oh, vxpt.UPSCALE_EASU_SHARPEN, 1.0)
        _assert_bits(got, vxpt.upscale_host(frame, ow, oh, vxpt.UPSCALE_EASU_SHARPEN, 1.0), "rendered frame")
        uw, uh, ms = r.upscale_info()
        assert (uw, uh) == (ow, oh) and ms > 0.0
        np.testing.assert_array_equal(r.read("FRAME"), frame)
        np.testing.assert_array_equal(r.read("OUTPUT"), output)
    finally:
        r.close()
