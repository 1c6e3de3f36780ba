"""Dynamic resolution on the GPU: vxpt_set_render_size (csrc/host_resize.cpp, csrc/resize.hip).  The resample
is compared bit for bit with vxpt_resize_host, which runs the same body on the host (and which
tests/test_resize.py compares with numpy); a context that resizes to its own size, or that was created larger
and set to a size before its first frame, must equal one that never heard of the feature; and the history
must survive a resize: the frame after it is closer to the converged image than a fresh context's first frame.
The world is the C1 terrain, (2, 1, 2) chunks, with the static C1 camera (ground below, sky above)."""
import numpy as np
import pytest

import vxpt
from golden.make_golden import C1_CAMERA

pytestmark = pytest.mark.gpu

# every buffer the inventory names as resampled, by its vxpt_buffer id: the denoiser's
# histories and history lengths, both reservoir parities, the last pass's slot (the next pass's taps and the
# current planes) with its tap records, the denoiser's history slot, the slot the last pass read
HISTORY = ("PREV_ILLUM", "PREV_FAST", "HIST_LEN", "PREV_HIST_LEN", "RES_EVEN", "RES_ODD",
           "DEPTH", "MATERIAL", "NORMAL_ROUGH", "GEO_NORMAL_THIN", "ALBEDO", "MAT_PARAM", "TAP_RECORD",
           "PREV_NORMAL_ROUGH", "PREV_DEPTH", "PREV_MATERIAL",
           "PREV_GEO_NORMAL_THIN", "PREV_ALBEDO", "PREV_MAT_PARAM")
ERR_ARG, ERR_STATE = -1, -4


def make(w, h, rows=None):
    r = vxpt.Renderer(w, h, rows=rows)
    r.load_settings()
    r.generate_terrain((2, 1, 2))
    r.set_camera(C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2], prev=C1_CAMERA)
    r.set_sky()
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d bytes differ" % (what, diff.sum(), diff.size)


def read_all(r, names=HISTORY):
    return {n: r.read(n) for n in names}


def test_resample_is_complete_and_bit_equal_to_the_host_twin():
    r = make(128, 96)
    try:
        assert r.render_size() == (128, 96, 128, 96)
        r.set_render_size(64, 48)
        assert r.render_size() == (64, 48, 128, 96)
        for f in range(3):
            r.render_frame(f, spp=2)
        before = read_all(r)
        assert before["DEPTH"].shape == (48, 64) and before["TAP_RECORD"].shape == (48, 64, 8)
        # the histories hold something: a resample of zeros would prove nothing
        for n in ("PREV_ILLUM", "PREV_FAST", "HIST_LEN", "PREV_HIST_LEN", "RES_EVEN", "RES_ODD", "DEPTH", "NORMAL_ROUGH",
                  "ALBEDO", "TAP_RECORD", "PREV_NORMAL_ROUGH", "PREV_DEPTH"):
            assert bits(before[n]).any(), n
        r.set_render_size(128, 96)
        for n in HISTORY:
            after = r.read(n)
            assert_bits(after, vxpt.resize_host(before[n], 128, 96), n)
            assert_bits(after, np.repeat(np.repeat(before[n], 2, axis=0), 2, axis=1), n + " (repeat)")
        # both parities as one buffer: the second starts at the new size's pixel count
        both = r.read("RESERVOIRS")
        assert_bits(both[:128 * 96].reshape(96, 128), vxpt.resize_host(before["RES_EVEN"], 128, 96), "RESERVOIRS even")
        assert_bits(both[128 * 96:].reshape(96, 128), vxpt.resize_host(before["RES_ODD"], 128, 96), "RESERVOIRS odd")
        r.render_frame(3, spp=2)  # and the context goes on at the new size
        assert np.isfinite(r.read("OUTPUT")).all()
    finally:
        r.close()


def test_resample_of_a_ragged_pair():
    """sizes that are no multiple of a tile or of each other, up and down again"""
    r = make(100, 74)
    try:
        r.set_render_size(50, 37)
        for f in range(3):
            r.render_frame(f, spp=2)
        small = read_all(r)
        r.set_render_size(83, 61)
        mid = read_all(r)
        for n in HISTORY:
            assert_bits(mid[n], vxpt.resize_host(small[n], 83, 61), n + " 50x37 -> 83x61")
        r.set_render_size(50, 37)
        for n in HISTORY:
            assert_bits(r.read(n), vxpt.resize_host(mid[n], 50, 37), n + " 83x61 -> 50x37")
        r.render_frame(3, spp=2)
        assert np.isfinite(r.read("OUTPUT")).all()
    finally:
        r.close()


def test_an_uploaded_motion_plane_is_resampled():
    r = make(64, 48)
    try:
        r.set_render_size(32, 24)
        motion = np.random.default_rng(5).standard_normal((24, 32, 4)).astype(np.float32)
        r.write("MOTION", motion)
        r.set_render_size(64, 48)
        assert_bits(r.read("MOTION"), vxpt.resize_host(motion, 64, 48), "MOTION")
    finally:
        r.close()


def test_setting_the_current_size_changes_nothing():
    a, b = make(64, 48), make(64, 48)
    try:
        names = HISTORY + ("OUTPUT", "ILLUM")
        for f in range(3):
            a.set_render_size(64, 48)
            a.render_frame(f, spp=2)
            b.render_frame(f, spp=2)
            for n in names:
                assert_bits(a.read(n), b.read(n), "%s after frame %d" % (n, f))
    finally:
        a.close()
        b.close()


def test_a_larger_context_set_to_a_size_equals_one_created_at_it():
    """catches every allocation, pitch or tile count still taken from the created size"""
    a, b = make(64, 48), make(128, 96)
    try:
        b.set_render_size(64, 48)  # before the first frame: only sets the size
        for f in range(3):
            a.render_frame(f, spp=2)
            b.render_frame(f, spp=2)
            for n in ("OUTPUT", "DEPTH", "RES_EVEN", "RES_ODD", "HIST_LEN", "PREV_ILLUM"):
                assert_bits(b.read(n), a.read(n), "%s after frame %d" % (n, f))
        a.postprocess()
        b.postprocess()
        assert_bits(b.read("FRAME"), a.read("FRAME"), "FRAME")
        assert b.row_bytes("OUTPUT") == a.row_bytes("OUTPUT") == 64 * 16
    finally:
        a.close()
        b.close()


def _rms(img, ref, mask):
    d = (img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64))[mask]
    return float(np.sqrt((d * d).mean()))


def test_history_survives_a_resize():
    """8 frames at 64x48, then one at 96x64 (another aspect ratio: the previous camera keeps the old view).
    Reference 1 is the converged image, 255 spp with every denoiser stage off; reference 2 a fresh context's
    frame 0 at 96x64 -- what destroying and creating the context gives.  The resized frame must be strictly
    closer to reference 1 than reference 2 is, and more than half of its non-sky pixels must carry a history
    longer than 1 frame.  An unresized 9-frame run at 96x64 has the history length above 1 in 0.988 of
    the non-sky pixels (the camera is static: what is missing are silhouette pixels the disocclusion test
    rejects), so the bar of one half leaves room; measured on one MI355X: the resized frame 0.975 of them, its
    RMS error 0.0200 against 0.0257 for the fresh frame 0."""
    spp = 1
    off = vxpt.DenoiseParams.defaults()
    for n in ("enable_temporal_accumulation", "enable_history_fix", "enable_history_clamping",
              "enable_spatial_filtering", "enable_firefly_filter"):
        setattr(off, n, 0)
    r = make(96, 64)
    try:
        r.render_frame(0, spp=255, params=off)
        ref1, depth = r.read("OUTPUT"), r.read("DEPTH")
    finally:
        r.close()
    mask = depth < 1e20
    assert 0.2 < mask.mean() < 0.95  # ground and sky
    r = make(96, 64)
    try:
        r.render_frame(0, spp=spp)
        ref2 = r.read("OUTPUT")
        for f in range(1, 9):
            r.render_frame(f, spp=spp)
        share_unresized = float((r.read("HIST_LEN")[mask] > 1.0).mean())
    finally:
        r.close()
    r = make(128, 96)
    try:
        r.set_render_size(64, 48)
        for f in range(8):
            r.render_frame(f, spp=spp)
        r.set_render_size(96, 64)
        r.render_frame(8, spp=spp)
        out, hist = r.read("OUTPUT"), r.read("HIST_LEN")
        mask &= r.read("DEPTH") < 1e20  # (the sub-pixel jitter moves the horizon's pixels between frames)
    finally:
        r.close()
    e_resized, e_fresh = _rms(out, ref1, mask), _rms(ref2, ref1, mask)
    share = float((hist[mask] > 1.0).mean())
    print("rms against 255 spp: resized frame %.5f, fresh frame 0 %.5f; history > 1 in %.3f of the non-sky pixels "
          "(unresized 9 frames: %.3f)" % (e_resized, e_fresh, share, share_unresized))
    assert share_unresized > 0.9
    assert e_resized < e_fresh
    assert share > 0.5


def test_refusals_leave_the_context_as_it_was():
    a, b = make(64, 48), make(64, 48)
    try:
        for w, h in ((65, 48), (64, 49), (0, 48), (64, -1)):
            with pytest.raises(vxpt.VxptError, match=r"\(%d\)" % ERR_ARG):
                a.set_render_size(w, h)
        assert a.render_size() == (64, 48, 64, 48) and (a.W, a.H) == (64, 48)
        a.render_frame(0, spp=2)
        b.render_frame(0, spp=2)
        for n in ("OUTPUT", "DEPTH", "RES_EVEN", "RES_ODD"):
            assert_bits(a.read(n), b.read(n), n)
    finally:
        a.close()
        b.close()
    a, b = make(64, 48, rows=(0, 24)), make(64, 48, rows=(0, 24))
    try:
        with pytest.raises(vxpt.VxptError, match=r"\(%d\)" % ERR_STATE):
            a.set_render_size(32, 24)
        assert a.render_size() == (64, 48, 64, 48)
        a.render_frame(0, spp=2)
        b.render_frame(0, spp=2)
        for n in ("OUTPUT", "DEPTH", "RES_EVEN", "RES_ODD"):
            assert_bits(a.read(n)[:24], b.read(n)[:24], n)
    finally:
        a.close()
        b.close()


def test_postprocess_and_upscale_follow_the_render_size():
    r = make(128, 96)
    try:
        r.render_frame(0, spp=2)
        r.postprocess()
        r.set_render_size(64, 48)
        r.render_frame(1, spp=2)
        r.postprocess()
        frame = r.read("FRAME")
        assert frame.shape == (48, 64, 4) and np.isfinite(frame).all() and frame[..., :3].std() > 0.01
        for mode in (vxpt.UPSCALE_BICUBIC, vxpt.UPSCALE_EASU_SHARPEN):
            up = r.upscale(128, 96, mode, 1.0)
            assert_bits(up, vxpt.upscale_host(frame, 128, 96, mode, 1.0), "upscale mode %d" % mode)
        with pytest.raises(vxpt.VxptError):
            r.upscale(63, 48)  # the lower bound follows the render size
        assert r.upscale(64, 48, vxpt.UPSCALE_BICUBIC).shape == (48, 64, 4)
        assert r.render_size_ms() > 0.0
    finally:
        r.close()


def _cam(r, which):
    """(pose and matrices, resolution fields, tan of the half fields of view) of vxpt_get_camera"""
    c = r.camera_info(which)
    return c[:24], c[24:28], c[28:30]


def test_the_previous_camera_keeps_the_old_view_for_one_frame():
    """After a resize that changes the aspect ratio the resampled history still shows the old size's view (the
    vertical field of view follows the ratio): the previous camera keeps that view at the new resolution until
    the frame's denoiser is enqueued -- by a frame call, or by a chain composed from single passes -- also when
    the camera moves in between; a resize that keeps the ratio changes the resolution fields alone."""
    fresh = make(96, 64)
    old = make(64, 48)
    try:
        new_view, new_res, new_tan = _cam(fresh, 1)
        old_view, _, old_tan = _cam(old, 1)
    finally:
        fresh.close()
        old.close()
    assert not np.array_equal(old_tan, new_tan)
    for end in ("frame", "passes", "moved"):
        r = make(128, 96)
        try:
            r.set_render_size(64, 48)
            r.render_frame(0, spp=1)
            r.set_render_size(96, 64)
            np.testing.assert_array_equal(_cam(r, 0)[0], new_view)  # the current camera: the new size's
            view, res, tan = _cam(r, 1)
            np.testing.assert_array_equal(res, new_res)
            np.testing.assert_array_equal(tan, old_tan)
            np.testing.assert_array_equal(view, old_view)
            if end == "frame":
                r.render_frame(1, spp=1)
            elif end == "passes":
                r.trace(1)
                r.denoise_pass(14)
            else:  # historyCamera = camera: the pose that rendered the history, still in the old view
                info = r.camera_info(0)
                r.set_camera_angles(C1_CAMERA[0], float(info[30]) + 0.05, float(info[31]), C1_CAMERA[2])
                np.testing.assert_array_equal(_cam(r, 1)[2], old_tan)
                np.testing.assert_array_equal(_cam(r, 1)[0], old_view)
                r.render_frame(1, spp=1)
            view, res, tan = _cam(r, 1)
            np.testing.assert_array_equal(tan, new_tan)
            np.testing.assert_array_equal(res, new_res)
            if end != "moved":
                np.testing.assert_array_equal(view, new_view)
        finally:
            r.close()
    r = make(128, 96)  # 128x96 -> 64x48: the same ratio, nothing is held
    try:
        r.render_frame(0, spp=1)
        before = _cam(r, 1)
        r.set_render_size(64, 48)
        after = _cam(r, 1)
        np.testing.assert_array_equal(after[0], before[0])
        np.testing.assert_array_equal(after[2], before[2])
        np.testing.assert_array_equal(after[1], np.float32([64, 48, 1 / 64, 1 / 48]))
    finally:
        r.close()
