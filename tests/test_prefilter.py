"""The denoiser's hit-distance reconstruction and pre-pass blur on the CPU: vxpt_prefilter_host runs the
per-pixel bodies of the gfx950 kernels (csrc/prefilter.hpp) on the host.  Tap coordinates against the
numpy evaluation (tests/prefilter_ref.py) exactly, both stages' values against it within a bar the test
measures itself, and the stages' pinned rules.

The bar: the reference is evaluated on the inputs with every hit distance, depth and
normal component moved by one fp32 ulp (three random sign patterns; the tap coordinates held); the
largest relative difference from the unperturbed reference, |a - b| / max(|b|, 1e-3), measures how far
the result moves when its inputs move by their own precision.  The bar is 4 x that figure: the margin
covers the body's handful of fp32 roundings per tap."""
import functools

import numpy as np
import pytest

import prefilter_ref as ref
import vxpt
from prefilter_ref import CAMERA, ITERATIONS, SHAPES

HIT, PRE = vxpt.PREFILTER_HIT_DIST, vxpt.PREFILTER_PRE_PASS
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _scene(w, h):
    return ref.scene(w, h)


def _host(stage, s, it=0, taps=False):
    return vxpt.prefilter_host(stage, s["illum"], s["depth"], s["normal_rough"], s["material"], s["camera"], it, taps)


def _ref(stage, s, it=0, coords=None):
    if stage == HIT:
        return ref.hitdist(s["illum"], s["depth"], s["normal_rough"])
    return ref.prepass(s["illum"], s["depth"], s["normal_rough"], s["material"], s["camera"], it, coords)


def _channels(stage):
    return slice(3, 4) if stage == HIT else slice(None)


def _bar(stage, s, it=0, coords=None):
    """4 x the reference's own movement under one-ulp nudges of its inputs"""
    base = _ref(stage, s, it, coords)
    worst = max(ref.rel_diff(_ref(stage, ref.nudge(s, seed), it, coords), base, _channels(stage)) for seed in (11, 12, 13))
    return 4.0 * worst, base


@functools.lru_cache(maxsize=None)
def _prepass_case(w, h, it):
    s = _scene(w, h)
    got, taps = _host(PRE, s, it, taps=True)
    bar, want = _bar(PRE, s, it, taps)
    return s, got, taps, bar, want


@pytest.mark.parametrize("it", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_tap_coordinates_equal_the_reference(shape, it):
    w, h = shape
    s, _, taps, _, _ = _prepass_case(w, h, it)
    want = ref.prepass_coords(s["illum"], s["depth"], s["camera"], it)
    assert taps.shape == (h, w, 8, 2)
    bad = np.argwhere(taps != want)
    assert bad.size == 0, (len(bad), bad[:5])
    # the case is live: taps inside and outside the screen, and radii beyond one texel
    inside = (taps[..., 0] >= 0) & (taps[..., 0] < w) & (taps[..., 1] >= 0) & (taps[..., 1] < h)
    ys, xs = np.mgrid[0:h, 0:w]
    reach = np.abs(taps - np.stack([xs, ys], -1)[:, :, None, :]).max()
    assert inside.any() and (~inside).any() and reach >= 8, (inside.mean(), reach)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_hit_distance_reconstruction_matches_reference(shape):
    w, h = shape
    s = _scene(w, h)
    got = _host(HIT, s)
    bar, want = _bar(HIT, s)
    err = ref.rel_diff(got, want, _channels(HIT))
    print("hitdist %dx%d: conditioning bar %.3e, host error %.3e" % (w, h, bar, err))
    assert np.isfinite(got).all()
    assert np.array_equal(got[..., :3], s["illum"][..., :3])  # the radiance passes through
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("it", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_pre_pass_matches_reference(shape, it):
    w, h = shape
    s, got, _, bar, want = _prepass_case(w, h, it)
    err = ref.rel_diff(got, want)
    print("prepass %dx%d it %d: conditioning bar %.3e, host error %.3e" % (w, h, it, bar, err))
    assert np.isfinite(got).all()
    assert err <= bar, (err, bar)
    # the blur is live: it changes the radiance of most pixels inside the range
    near = s["depth"] <= ref.RANGE
    assert (np.abs(got[..., :3] - s["illum"][..., :3]).max(-1)[near] > 1e-3).mean() > 0.5


# ---------------------------------------------------------------- pinned rules
def test_skipped_sky_pixels_pass_through():
    s = _scene(50, 29)
    sky = s["depth"] > ref.RANGE
    assert sky.any() and (~sky).any()
    for stage in (HIT, PRE):
        got = _host(stage, s, 1)
        assert np.array_equal(got[sky], s["illum"][sky]), stage


def _flat_scene(w, h, depth, hit=7.0, radiance=(0.3, 0.7, 0.125)):
    """one plane facing the camera, `depth` in front of it, one material, constant radiance and hit distance"""
    ys, xs = np.mgrid[0:h, 0:w]
    _, d = ref.ray_dirs(CAMERA, w, h, xs.astype(np.float64), ys.astype(np.float64))
    fwd = np.asarray(CAMERA[1], np.float64)
    fwd /= np.linalg.norm(fwd)
    nr = np.concatenate([np.broadcast_to(-fwd, (h, w, 3)), np.full((h, w, 1), 0.8)], -1)
    il = np.empty((h, w, 4))
    il[..., :3] = radiance
    il[..., 3] = hit
    return dict(illum=il.astype(np.float32), depth=(depth / (d @ fwd)).astype(np.float32),
                normal_rough=nr.astype(np.float32), material=np.full((h, w), 3.0, np.float32), camera=CAMERA)


def test_reconstruction_gives_a_zero_centre_no_weight():
    s = _flat_scene(21, 17, 20.0)
    s["illum"][8, 10, 3] = 0.0
    got = _host(HIT, s)
    # the neighbours all hold 7: with the centre's weight 0 their average is 7; a centre weight of
    # 1000 would drag the result to nearly 0
    assert abs(got[8, 10, 3] - 7.0) <= 7.0 * 1e-6, got[8, 10, 3]
    # and a non-zero centre dominates with its weight of 1000
    s["illum"][8, 10, 3] = 1.0
    got = _host(HIT, s)
    assert 1.0 < got[8, 10, 3] < 1.1, got[8, 10, 3]


def test_pre_pass_radius_is_at_least_one_for_a_zero_hit_distance():
    # so far away that 30 * saturate(1 / frustumSize) is a hundredth of a texel
    w, h, it = 33, 21, 7
    far = _flat_scene(w, h, 2000.0, hit=1.0)
    _, taps = _host(PRE, far, it, taps=True)
    ys, xs = np.mgrid[0:h, 0:w]
    own = np.stack([xs, ys], -1)[:, :, None, :]
    assert (taps == own).all()  # hit distance 1: every tap falls on the pixel itself
    zero = _flat_scene(w, h, 2000.0, hit=0.0)
    _, taps = _host(PRE, zero, it, taps=True)
    ca, sa = ref.rotator(it)
    F = np.float32
    for i in range(8):
        ox, oy = ref.POISSON8[i, 0], ref.POISSON8[i, 1]
        rx, ry = F(ox * ca) + F(oy * sa), F(ox * F(-sa)) + F(oy * ca)
        want = np.stack([np.floor(xs + 0.5 + float(rx) * 1.0), np.floor(ys + 0.5 + float(ry) * 1.0)], -1)
        assert (taps[:, :, i] == want).all(), i
    assert (taps != own).any()


def test_pre_pass_keeps_a_constant_radiance():
    """every tap holds the centre's radiance, so the weighted mean is that radiance; the bar is the
    pre-pass's measured one for the 50x29 planes at the same iteration"""
    w, h, it = 50, 29, 1
    bar = _prepass_case(w, h, it)[3]
    s = _flat_scene(w, h, 20.0)
    rng = np.random.default_rng(5)
    s["illum"][..., 3] = (50.0 * (1.0 - rng.random((h, w)))).astype(np.float32)
    got, taps = _host(PRE, s, it, taps=True)
    err = ref.rel_diff(got[..., :3], s["illum"][..., :3])
    print("constant radiance: error %.3e, bar %.3e" % (err, bar))
    assert err <= bar, (err, bar)
    # live: taps with a non-zero weight exist (the w channel gathers the weight sum, > 1 then)
    assert (got[..., 3] - s["illum"][..., 3] > 1.5).mean() > 0.5


def test_last_column_tap_reads_its_own_texel_geometry():
    """The reference rounds its G-buffer position to texel k + 1 (PrePass.h:105); on the last column that
    is texel W, which a row-major plane holds as column 0 of the next row.  Here geometry and radiance
    both come from texel k: column 0's material must not reach a pixel whose taps stay right of it."""
    w, h, it = 50, 29, 1
    s = _flat_scene(w, h, 20.0, hit=40.0)
    s["illum"][:, w - 1, :3] = 10.0  # the last column's radiance stands out
    a = dict(s)
    b = dict(s)
    b["material"] = s["material"].copy()
    b["material"][:, 0] = 9.0  # texel W of a row = column 0 of the next one: another material
    got_a, taps = _host(PRE, a, it, taps=True)
    got_b = _host(PRE, b, it)
    right = slice(w - 16, w)
    lands = (taps[:, right, :, 0] == w - 1) & (taps[:, right, :, 1] >= 0) & (taps[:, right, :, 1] < h)
    assert lands[:, :-1].any()  # taps of other columns' pixels land on the last column
    assert (taps[:, right, :, 0] > 0).all()  # and none of them reaches column 0
    assert np.array_equal(got_a[:, right], got_b[:, right])
    # those taps count, with the last column's own material and radiance
    want = _ref(PRE, a, it, taps)
    assert ref.rel_diff(got_a[:, right], want[:, right]) <= _prepass_case(w, h, it)[3]
    hit = lands[:, :-1].any(-1)
    assert (got_a[:, right][:, :-1][hit][..., 0] > s["illum"][0, 0, 0] + 0.1).any()


def test_argument_checks():
    s = _scene(24, 20)
    with pytest.raises(vxpt.VxptError):
        _host(2, s)
    lib = vxpt.load_library()
    assert lib.vxpt_prefilter_host(0, 0, 4, None, 0, None, None, None, None, None, None) == -1


def test_denoise_params_trailing_fields_default_to_off():
    old = vxpt.DenoiseParams(30.0, 6.0, 2.0, 0.5, 0.15, 0.003, 0.01, 0.05, 500000.0, 1, 1, 1, 1, 1, 1)
    assert old.enable_hit_distance_reconstruction == 0 and old.enable_pre_pass == 0
    d = vxpt.DenoiseParams.defaults()
    assert bytes(d) == bytes(old)


def test_band_schedule_refuses_the_switches():
    """bands.py composes the banded chain from single passes and has no halo group for the two stages"""
    import bands
    assert bands.params_dict(vxpt.DenoiseParams.defaults())["ta"]
    for name in ("enable_hit_distance_reconstruction", "enable_pre_pass"):
        p = vxpt.DenoiseParams.defaults()
        setattr(p, name, 1)
        with pytest.raises(ValueError, match=name):
            bands.params_dict(p)
