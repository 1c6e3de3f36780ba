"""The denoiser's hit-distance reconstruction (pass 15, k_hitdist) and pre-pass blur (pass 16, k_prepass)
on the GPU: the single passes against the same bodies on the host, the frame calls against the chain
composed from single passes, the pipelined run against frame calls, the switches' off state against the
parameter struct built without them, the settings keys, and the refusal on banded contexts."""
import os

import numpy as np
import pytest

import bands
import prefilter_ref as ref
import vxpt
from golden.make_golden import C1_CAMERA

pytestmark = pytest.mark.gpu

BUFS = ("ILLUM", "PING", "PONG", "PREV_ILLUM", "PREV_FAST", "HIST_LEN", "PREV_HIST_LEN", "OUTPUT")
OLD_15 = (30.0, 6.0, 2.0, 0.5, 0.15, 0.003, 0.01, 0.05, 500000.0, 1, 1, 1, 1, 1, 1)


def _params(recon, pre):
    p = vxpt.DenoiseParams.defaults()
    p.enable_hit_distance_reconstruction, p.enable_pre_pass = int(recon), int(pre)
    return p


def _c1(w=128, h=96):
    r = vxpt.Renderer(w, h)
    r.load_settings()
    r.generate_terrain((2, 1, 2))
    r.set_camera(C1_CAMERA[0], C1_CAMERA[1], fov=C1_CAMERA[2], prev=C1_CAMERA)
    r.set_sky()
    return r


def _state(r):
    return {b: r.read(b) for b in BUFS}


def _same(a, b, tag):
    for name in BUFS:
        x, y = a[name], b[name]
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (tag, name, float(np.abs(x - y).max()))


# ---------------------------------------------------------------- 1. single passes against the host bodies
@pytest.mark.parametrize("shape", ref.SHAPES, ids=["%dx%d" % s for s in ref.SHAPES])
def test_single_passes_match_the_host_bodies(shape):
    w, h = shape
    s = ref.scene(w, h)
    cam = s["camera"]
    r = vxpt.Renderer(w, h)
    try:
        r.set_camera(cam[0], cam[1], fov=cam[2], prev=cam)
        host = lambda stage, illum, it=0: vxpt.prefilter_host(stage, illum, s["depth"], s["normal_rough"], s["material"],
                                                              cam, it)

        def upload(illum):
            r.write("ILLUM", illum)
            r.write("DEPTH", s["depth"])
            r.write("NORMAL_ROUGH", s["normal_rough"])
            r.write("MATERIAL", s["material"])

        def check(got, want, tag):
            err = ref.rel_diff(got, want)
            print("%s %dx%d: device vs host %.3e" % (tag, w, h, err))
            assert np.isfinite(got).all()
            assert err <= 1e-4, (tag, err)

        upload(s["illum"])
        r.denoise_pass(15)
        recon = r.read("PING")
        want_recon = host(vxpt.PREFILTER_HIT_DIST, s["illum"])
        check(recon, want_recon, "pass 15")
        assert np.array_equal(r.read("ILLUM"), s["illum"])  # its input is left alone
        for it in ref.ITERATIONS:
            # input 1: the reconstruction's output in the ping plane
            r.write("PING", recon)
            r.denoise_pass(16, it, 1)
            check(r.read("ILLUM"), host(vxpt.PREFILTER_PRE_PASS, recon, it), "pass 16 from ping, it %d" % it)
            # input 0: the radiance itself (not in place: it travels through the ping plane)
            upload(s["illum"])
            r.denoise_pass(16, it, 0)
            check(r.read("ILLUM"), host(vxpt.PREFILTER_PRE_PASS, s["illum"], it), "pass 16 from illum, it %d" % it)
    finally:
        r.close()


# ---------------------------------------------------------------- 2. frame call against composed passes
def _composed_frame(r, f, p):
    """the frame's trace and the chain in the reference's order, one vxpt_denoise_pass at a time"""
    recon, pre = bool(p.enable_hit_distance_reconstruction), bool(p.enable_pre_pass)
    off = vxpt.DenoiseParams.from_buffer_copy(p)  # the band schedule's switches: it knows nothing of the two stages
    off.enable_hit_distance_reconstruction = off.enable_pre_pass = 0
    it = f + 1
    inserted = False
    for op in bands.frame_ops(f, 1, bands.params_dict(off)):
        if op[0] == "trace":
            r.trace_flags(op[1], op[2])
        elif op[0] == "pass":
            which, arg, arg2 = op[1:4]
            if which in (12, 2, 5, 13) and not inserted:
                # firefly -> reconstruction -> pre-pass -> frame-0 init -> temporal accumulation -> ...
                inserted = True
                if recon:
                    r.denoise_pass(15, 0, 0, p)
                if pre:
                    r.denoise_pass(16, it, 1 if recon else 0, p)
            if which == 13 and arg == 0 and recon:
                arg = 1  # Denoiser.cu:91: the reconstruction alone moves the result to the ping plane
            r.denoise_pass(which, arg, arg2, p)
    assert inserted


def _chain_params(recon, pre, plain):
    p = _params(recon, pre)
    if plain:  # no temporal accumulation, no spatial filter: the output comes straight from the source plane
        p.enable_temporal_accumulation = p.enable_history_fix = p.enable_history_clamping = 0
        p.enable_spatial_filtering = 0
    return p


@pytest.mark.parametrize("recon,pre,plain", [(1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 0, 1), (1, 1, 1)],
                         ids=["both", "reconstruction", "pre-pass", "reconstruction-plain", "both-plain"])
def test_frame_call_equals_composed_passes(recon, pre, plain):
    """plain = the chain without temporal accumulation and spatial filtering: nothing overwrites the ping
    plane after the reconstruction, so a frame call that left k_hitdist out, or took its output from
    illum instead of ping (the output-source rule), differs from the composed chain."""
    p = _chain_params(recon, pre, plain)
    a, b = _c1(), _c1()
    try:
        for f in range(3):
            a.render_frame(f, 1, p)
            _composed_frame(b, f, p)
            sa = _state(a)
            _same(sa, _state(b), "frame %d" % f)
            if plain:
                # the output is the ping plane's radiance times the albedo (sky: the radiance itself), and
                # the ping plane holds this frame's reconstruction: its w is not the radiance's everywhere
                ping, alb, sky = sa["PING"], a.read("ALBEDO"), a.read("DEPTH") > 500000.0
                want = np.where(sky[..., None], sa["ILLUM"][..., :3], ping[..., :3] * alb[..., :3])
                assert np.array_equal(sa["OUTPUT"][..., :3], want)
                assert (ping[..., 3][~sky] != a.read("ILLUM")[..., 3][~sky]).any() or pre
                if pre:  # the pre-pass blurred illum, the output still comes from ping: they differ
                    assert not np.array_equal(sa["ILLUM"][..., :3][~sky], ping[..., :3][~sky])
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 3. pipelined run
def test_pipelined_frames_equal_frame_calls():
    p = _params(1, 1)
    a, b = _c1(), _c1()
    try:
        a.render_frames(0, 3, 2, p)
        for f in range(3):
            b.render_frame(f, 2, p)
        _same(_state(a), _state(b), "3 frames, 2 spp")
        assert a.timings()["denoise_ms"] > 0
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 4. off is the parent
def test_off_equals_the_struct_built_without_the_fields():
    old = vxpt.DenoiseParams(*OLD_15)
    off, on = _params(0, 0), _params(0, 1)
    rs = [_c1() for _ in range(3)]
    try:
        for r, p in zip(rs, (old, off, on)):
            for f in range(3):
                r.render_frame(f, 1, p)
        so, sf, sn = (_state(r) for r in rs)
        _same(so, sf, "off vs 15 positional values")
        assert not np.array_equal(sn["OUTPUT"], sf["OUTPUT"])  # the pre-pass does change the image
    finally:
        for r in rs:
            r.close()


# ---------------------------------------------------------------- 5. settings
def test_settings_keys_are_read(tmp_path):
    src = os.path.join(vxpt.DATA_DIR, "settings", "global_settings.yaml")
    text = open(src).read()
    assert "enableHitDistanceReconstruction: false" in text and "enablePrePass: false" in text
    r = vxpt.Renderer(64, 48)
    try:
        r.load_settings()
        d = r.denoise_params()
        assert (d.enable_hit_distance_reconstruction, d.enable_pre_pass) == (0, 0)
    finally:
        r.close()
    # a data directory whose settings file turns both on; everything else is the repository's
    for name in os.listdir(vxpt.DATA_DIR):
        if name != "settings":
            os.symlink(os.path.join(vxpt.DATA_DIR, name), tmp_path / name)
    (tmp_path / "settings").mkdir()
    for name in os.listdir(os.path.dirname(src)):
        if name != "global_settings.yaml":
            os.symlink(os.path.join(os.path.dirname(src), name), tmp_path / "settings" / name)
    (tmp_path / "settings" / "global_settings.yaml").write_text(
        text.replace("enableHitDistanceReconstruction: false", "enableHitDistanceReconstruction: true")
            .replace("enablePrePass: false", "enablePrePass: true"))
    r = vxpt.Renderer(64, 48, data_dir=str(tmp_path))
    try:
        r.load_settings()
        d = r.denoise_params()
        assert (d.enable_hit_distance_reconstruction, d.enable_pre_pass) == (1, 1)
        assert d.enable_temporal_accumulation == 1 and d.atrous_iteration_num == vxpt.DenoiseParams.defaults().atrous_iteration_num
    finally:
        r.close()


# ---------------------------------------------------------------- 6. bands
def test_banded_calls_refuse_the_switches():
    w, h = 96, 160
    rs = [_c1(w, h) for _ in range(2)]
    try:
        linked = vxpt.LinkedBands(rs)
        lib = vxpt.load_library()
        import ctypes
        for p in (_params(0, 1), _params(1, 0)):
            rc = lib.vxpt_render_frame_linked(linked._arr, 2, ctypes.byref(p), 0, 1)
            assert rc == -4, rc  # VXPT_ERR_STATE
            msg = lib.vxpt_last_error(rs[0].ctx).decode()
            assert ("enable_pre_pass" if p.enable_pre_pass else "enable_hit_distance_reconstruction") in msg, msg
            assert lib.vxpt_render_frames_linked(linked._arr, 2, ctypes.byref(p), 0, 2, 1) == -4
        on = _params(0, 1)
        for call in (lambda: rs[0].denoise_pass(16, 1, 0),        # a member of the group, on its own
                     lambda: rs[0].denoise_pass(5, 0, 0, on),     # any pass of a chain composed with the switch on
                     lambda: rs[0].render_frame(0, 1, on),
                     lambda: rs[0].render_frames(0, 2, 1, on),
                     lambda: rs[0].denoise(0, 1, on)):
            with pytest.raises(vxpt.VxptError, match="enable_pre_pass"):
                call()
        # the contexts still render with the switches off
        single = _c1(w, h)
        try:
            off = _params(0, 0)
            linked.render_frame(0, 1, off)
            single.render_frame(0, 1, off)
            rows = [bands.band_rows(h, 2, k) for k in range(2)]
            out = np.concatenate([r.read("OUTPUT")[y0:y1] for r, (y0, y1) in zip(rs, rows)])
            assert np.array_equal(out.view(np.uint32), single.read("OUTPUT").view(np.uint32))
        finally:
            single.close()
    finally:
        for r in rs:
            r.close()


def test_row_range_context_is_refused_and_left_untouched():
    """A context with only a row range: the frame calls refuse a switch before anything is enqueued, so the
    context then renders what a fresh one renders."""
    w, h, y1 = 128, 96, 48
    refused, fresh = _c1(w, h), _c1(w, h)
    try:
        for r in (refused, fresh):
            r.set_band(0, y1)
        off = _params(0, 0)
        for p in (_params(0, 1), _params(1, 0)):
            name = "enable_pre_pass" if p.enable_pre_pass else "enable_hit_distance_reconstruction"
            with pytest.raises(vxpt.VxptError, match=name):
                refused.render_frame(0, 2, p)
            with pytest.raises(vxpt.VxptError, match=name):
                refused.render_frames(0, 3, 2, p)
            with pytest.raises(vxpt.VxptError, match=name):
                refused.denoise_pass(15 if p.enable_hit_distance_reconstruction else 16, 1, 0, p)
        for f in range(2):
            refused.render_frame(f, 2, off)
            fresh.render_frame(f, 2, off)
        refused.render_frames(2, 2, 2, off)
        fresh.render_frames(2, 2, 2, off)
        _same(_state(refused), _state(fresh), "after the refusals")
        for name in ("DEPTH", "NORMAL_ROUGH", "RESERVOIRS"):
            assert refused.read(name).tobytes() == fresh.read(name).tobytes(), name
    finally:
        refused.close()
        fresh.close()
