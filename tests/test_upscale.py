"""Render scale on the CPU: vxpt_upscale_host runs the per-pixel bodies of the gfx950 kernels
(csrc/upscale.hpp) on the host.  Parity with the float64 numpy evaluation (tests/upscale_ref.py),
properties that need no reference, and the argument checks."""
import ctypes

import numpy as np
import pytest

import upscale_ref as ref
import vxpt
from upscale_ref import BAR, MODES, SHAPES

MODE_NAMES = {0: "bicubic", 1: "easu", 2: "easu-sharp"}


def _images(w, h):
    return {"noise": ref.noise_image(w, h, seed=w * 1000 + h), "smooth": ref.smooth_image(w, h)}


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-%dx%d" % (a + b) for a, b in SHAPES])
def test_host_matches_numpy_reference(shape, mode):
    (w, h), (ow, oh) = shape
    for name, img in _images(w, h).items():
        got = vxpt.upscale_host(img, ow, oh, mode, 1.0)
        want = ref.upscale(img, ow, oh, mode, 1.0)
        assert got.shape == (oh, ow, 4) and got.dtype == np.float32
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - want).max()
        print("%s %s %dx%d -> %dx%d: max abs error %.3e" % (MODE_NAMES[mode], name, w, h, ow, oh, err))
        assert err < BAR, (name, err)
        assert (got[..., 3] == 0.0).all()


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_sharpness_parity_below_one(mode):
    """the sharpness parameter itself (the reference fixes it at 1)"""
    img = ref.smooth_image(37, 23)
    for sharp in (0.0, 0.35):
        got = vxpt.upscale_host(img, 64, 40, mode, sharp)
        assert np.abs(got - ref.upscale(img, 64, 40, mode, sharp)).max() < BAR


@pytest.mark.parametrize("mode", MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_constant_image_is_reproduced_exactly(mode):
    for value in ((0.3, 0.7, 0.123456), (0.0, 1.0, 0.5), (1e-3, 0.9999, 0.6180339)):
        img = np.empty((23, 37, 4), np.float32)
        img[..., :3] = np.float32(value)
        img[..., 3] = 0.25
        for ow, oh in ((64, 40), (37, 23), (74, 46)):
            got = vxpt.upscale_host(img, ow, oh, mode, 1.0)
            np.testing.assert_array_equal(got[..., :3], np.broadcast_to(np.float32(value), (oh, ow, 3)))


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-%dx%d" % (a + b) for a, b in SHAPES])
def test_easu_stays_inside_its_four_nearest_texels(shape):
    (w, h), (ow, oh) = shape

    def anchors(n_in, n_out):  # the documented mapping, in the library's fp32
        s = np.float32(n_in) / np.float32(n_out)
        p = np.arange(n_out, dtype=np.float32) * s + (np.float32(0.5) * s - np.float32(0.5))
        return np.floor(p).astype(np.int64)

    ax, ay = anchors(w, ow), anchors(h, oh)
    for name, img in _images(w, h).items():
        got = vxpt.upscale_host(img, ow, oh, ref.EASU, 1.0)[..., :3]
        quad = np.stack([img[np.clip(ay + dy, 0, h - 1)[:, None], np.clip(ax + dx, 0, w - 1)[None, :], :3]
                         for dy in (0, 1) for dx in (0, 1)])
        assert (got >= quad.min(axis=0)).all() and (got <= quad.max(axis=0)).all(), name


def test_sharpness_acts_on_edges_and_not_on_flat_regions():
    w, h, ow, oh = 32, 12, 64, 24
    img = np.zeros((h, w, 4), np.float32)
    img[:, : w // 2, :3] = (0.2, 0.3, 0.25)
    img[:, w // 2:, :3] = (0.7, 0.6, 0.8)
    soft = vxpt.upscale_host(img, ow, oh, ref.EASU_SHARPEN, 0.0)
    hard = vxpt.upscale_host(img, ow, oh, ref.EASU_SHARPEN, 1.0)
    edge = slice(ow // 2 - 4, ow // 2 + 4)
    assert np.abs(soft[:, edge] - hard[:, edge]).max() > 1e-3
    # 8 output pixels (4 texels) from the step, every tap of either filter sees one constant
    for flat, value in ((slice(0, ow // 2 - 8), (0.2, 0.3, 0.25)), (slice(ow // 2 + 8, ow), (0.7, 0.6, 0.8))):
        np.testing.assert_array_equal(soft[:, flat], hard[:, flat])
        np.testing.assert_array_equal(soft[:, flat, :3], np.broadcast_to(np.float32(value), soft[:, flat, :3].shape))


def test_easu_is_transposition_equivariant():
    """upscale(img.T) == upscale(img).T: catches an x/y mix-up of the luminance slots or the taps."""
    w, h, ow, oh = 37, 23, 64, 40
    img = ref.smooth_image(w, h)
    img_t = np.ascontiguousarray(img.transpose(1, 0, 2))
    # preconditions on the float64 evaluation: the zero-gradient fallback direction (1, 0), which is
    # not equivariant, fires nowhere on this image, and the evaluation itself is equivariant
    want, fallback = ref.easu(img, ow, oh, return_fallback=True)
    want_t, fallback_t = ref.easu(img_t, oh, ow, return_fallback=True)
    assert not fallback.any() and not fallback_t.any()
    assert np.abs(want_t - want.transpose(1, 0, 2)).max() < 1e-6
    got = vxpt.upscale_host(img, ow, oh, ref.EASU, 1.0)
    got_t = vxpt.upscale_host(img_t, oh, ow, ref.EASU, 1.0)
    err = np.abs(got_t - got.transpose(1, 0, 2)).max()
    print("transposition: max abs difference %.3e" % err)
    assert err < BAR


def test_argument_checks():
    lib = vxpt.load_library()
    img = ref.noise_image(8, 6)
    out = np.zeros((32, 32, 4), np.float32)

    def call(w, h, ow, oh, mode, sharp):
        return lib.vxpt_upscale_host(img.ctypes.data, w, h, out.ctypes.data, ow, oh, mode, ctypes.c_float(sharp))

    ERR_ARG = -1
    assert call(8, 6, 16, 12, 2, 1.0) == 0
    assert call(8, 6, 7, 12, 1, 1.0) == ERR_ARG   # narrower than the input
    assert call(8, 6, 16, 5, 1, 1.0) == ERR_ARG   # shorter than the input
    assert call(8, 6, 16, 12, 3, 1.0) == ERR_ARG  # unknown modes
    assert call(8, 6, 16, 12, -1, 1.0) == ERR_ARG
    for sharp in (-0.01, 1.01, float("nan")):
        assert call(8, 6, 16, 12, 2, sharp) == ERR_ARG
    assert call(0, 6, 16, 12, 1, 1.0) == ERR_ARG  # non-positive input sizes
    assert call(8, -6, 16, 12, 1, 1.0) == ERR_ARG
    with pytest.raises(vxpt.VxptError):
        vxpt.upscale_host(img, 4, 4)
