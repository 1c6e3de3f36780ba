"""GPU: the denoiser's passes one at a time on the synthetic edge frames of tests/denoise_frames.py.

(a) every pass against the oracle's pass on the same planes; every plane the pass does not write must come back
    byte for byte;
(b) the three a-trous kernels (k_atrous_smem, k_atrous and its final variant) against the float64 restatement
    tests/denoise_ref.py, at the bar the oracle itself keeps against it (test_denoise_ref.ORACLE_VS_F64);
(c) the denoiser-side tuning fields change no bit of any pass's result on these frames;
(d) the whole chain against the oracle over the switch settings;
(e) history lengths injected around the two accumulation caps, three chained frames.
"""
import numpy as np
import pytest

import denoise_frames
import denoise_ref
import vxpt
from test_denoise_ref import AMBIGUOUS_CAP, DEPTH_THR, FRAME_INDEX, LOBE, ORACLE_VS_F64, PHI, SEED
from test_gpu_parity import DN_FLOATS, DN_INTS, RTOL_DN, _dn_params, _inject_frame, _rel, _setup

pytestmark = pytest.mark.gpu

WATCHED = denoise_frames.PLANES + ("OUTPUT",)
RES_FIELDS = ("lightData", "uvData", "weightSum", "targetPdf", "M")
STEPS = (2, 4, 8, 16, 32, 64)
COPY_SRC = {0: "ILLUM", 1: "PING", 2: "PONG", 3: "PREV_ILLUM"}
# label -> (GPU passes [(id, arg, arg2)], oracle passes, planes written); pass 11 (world positions) runs first where
# include/vxpt.h says so; the history fix walks the lists the temporal pass leaves, so it runs behind it
SEQUENCE = {}
for par in (0, 1):
    SEQUENCE["firefly%d" % par] = ([(0, par, 0)], [(0, par, 0)], ("ILLUM", "RESERVOIRS"))
SEQUENCE["temporal"] = ([(2, 0, 0)], [(2, 0, 0)], ("PING", "PONG", "HIST_LEN"))
SEQUENCE["history_fix"] = ([(11, 0, 0), (2, 0, 0), (3, 0, 0)], [(2, 0, 0), (3, 0, 0)], ("PING", "PONG", "HIST_LEN"))
SEQUENCE["history_clamp"] = ([(4, 0, 0)], [(4, 0, 0)], ("PREV_ILLUM", "PREV_FAST", "PREV_HIST_LEN"))
SEQUENCE["atrous_first"] = ([(11, 0, 0), (5, 0, 0)], [(5, 0, 0)], ("PING",))
for st in STEPS:
    SEQUENCE["atrous6_%d" % st] = ([(11, 0, 0), (6, st, FRAME_INDEX)], [(6, st, FRAME_INDEX)], ("PONG",))
    SEQUENCE["atrous7_%d" % st] = ([(11, 0, 0), (7, st, FRAME_INDEX)], [(7, st, FRAME_INDEX)], ("PING",))
    SEQUENCE["atrous10_%d" % st] = ([(11, 0, 0), (10, st, FRAME_INDEX)],
                                    [(6, st, FRAME_INDEX), (1, 0, 0), (8, vxpt.BUF["PONG"], 0)], ("PONG", "OUTPUT"))
SEQUENCE["frame0_init"] = ([(12, 0, 0)], [(10, 0, 0)], ("PREV_ILLUM", "PREV_FAST", "HIST_LEN", "PREV_HIST_LEN"))
for src, name in COPY_SRC.items():
    SEQUENCE["copy_%d" % src] = ([(13, src, 0)], [(1, 0, 0), (8, vxpt.BUF[name], 0)], ("OUTPUT",))


class Side:
    """A renderer / oracle pair at one size, the synthetic frame and what each label's passes leave."""

    def __init__(self, w, h, tuning=None, with_oracle=True):
        self.w, self.h = w, h
        self.r, self.o = _setup(w, h)
        if tuning:
            self.r.set_tuning(**tuning)
        self.r.trace(0)  # establishes the G-buffer ring slots; every plane is overwritten below
        self.cam = self.r.camera_info(0)
        self.planes = denoise_frames.make(w, h, SEED, cam=self.cam)
        self.planes["OUTPUT"] = np.full((h, w, 4), 0.375, np.float32)
        self.p = _dn_params()
        self.with_oracle = with_oracle
        self.results = {}

    def inject(self):
        for name in WATCHED:
            self.r.write(name, self.planes[name])
            if self.with_oracle:
                self.o.write(vxpt.BUF[name], self.planes[name])

    def run(self, label):
        """(GPU planes before the passes, after them, the oracle's planes after its passes)"""
        if label not in self.results:
            gpu, orc, _ = SEQUENCE[label]
            self.inject()
            before = {n: self.r.read(n) for n in WATCHED}
            for which, arg, arg2 in gpu:
                self.r.denoise_pass(which, arg, arg2, self.p)
            after = {n: self.r.read(n) for n in WATCHED}
            ref = None
            if self.with_oracle:
                for which, arg, arg2 in orc:
                    self.o.run_pass(which, arg, arg2)
                ref = {n: self.o.read(vxpt.BUF[n]) for n in WATCHED}
            self.results[label] = (before, after, ref)
        return self.results[label]

    def close(self):
        self.r.close()


@pytest.fixture(scope="module", params=denoise_frames.SIZES, ids=lambda s: "%dx%d" % s)
def side(request):
    """One renderer per size for the module (a size the library refused would fail here, for every test of it)."""
    w, h = request.param
    s = Side(w, h)
    yield s
    s.close()


def test_camera_and_sky_depth_match_the_builder(side):
    """The frame was built for the renderer's own camera; the oracle's equals it; the trace writes the builder's sky
    depth; and every plane reads back as written (PING, PONG and OUTPUT included)."""
    np.testing.assert_allclose(side.cam[:30], side.o.camera_info(0)[:30], rtol=0, atol=2e-7)  # test_camera_matrices' bar
    side.r.trace(0, primary_only=True)
    d = side.r.read("DEPTH")
    assert (d[d > 5e5] == denoise_frames.SKY_DEPTH).all()
    side.inject()
    for n in WATCHED:
        got = side.r.read(n)
        for fld in (RES_FIELDS if n == "RESERVOIRS" else (None,)):
            a, b = (got, side.planes[n]) if fld is None else (got[fld], side.planes[n][fld])
            np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8), err_msg=n)


def _same_bytes(a, b, what):
    if a.dtype.names:
        for fld in RES_FIELDS:
            np.testing.assert_array_equal(a[fld].view(np.uint32), b[fld].view(np.uint32), err_msg="%s %s" % (what, fld))
    else:
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


@pytest.mark.parametrize("label", list(SEQUENCE))
def test_pass_against_oracle(side, label):
    before, after, ref = side.run(label)
    written = SEQUENCE[label][2]
    for n in WATCHED:
        what = "%s %dx%d %s" % (label, side.w, side.h, n)
        if n in written and n != "RESERVOIRS":  # the pass ran: it left something other than what was written in
            assert (after[n] != before[n]).any(), what
        if n not in written:
            _same_bytes(after[n], before[n], what + " (not written by the pass)")
        elif n == "RESERVOIRS":
            _same_bytes(after[n], ref[n], what)
        elif n in ("HIST_LEN", "PREV_HIST_LEN"):
            print(what, "max abs diff", np.abs(after[n] - ref[n]).max())
            np.testing.assert_array_equal(after[n], ref[n], err_msg=what)
        elif n == "ILLUM":  # the firefly filter's pixels: the same set, values within 1e-5
            np.testing.assert_array_equal((after[n] != before[n]).any(-1), (ref[n] != side.planes[n]).any(-1), err_msg=what)
            rel = _rel(after[n], ref[n])
            print(what, "max rel", rel.max())
            assert rel.max() < 1e-5, (what, rel.max())
        else:
            rel = _rel(after[n], ref[n])
            print(what, "max rel", rel.max())
            assert np.isfinite(after[n]).all(), what
            assert rel.max() < RTOL_DN, (what, rel.max(), np.unravel_index(rel.argmax(), rel.shape))
    if label.startswith("firefly"):  # every outlier fired
        half = side.w * side.h
        par = int(label[-1])
        ws = after["RESERVOIRS"]["weightSum"][par * half:(par + 1) * half].reshape(side.h, side.w)
        for (y, x) in side.planes["_outliers"]:
            assert ws[y, x] < side.planes["RESERVOIRS"]["weightSum"][par * half + y * side.w + x], (y, x)


def _against_f64(side, got, ref, what):
    out, written, amb = ref
    geo = ~side.planes["_sky"]
    frac = amb[geo].mean()
    assert frac <= AMBIGUOUS_CAP, (what, "ambiguous fraction", frac)
    use = written & ~amb
    e = _rel(got.astype(np.float64), out)[use]
    k = np.argwhere(use)[e.max(-1).argmax()]
    print("%s %dx%d: GPU vs float64 max rel %.3e at (y, x) %s, ambiguous %.4f" % (what, side.w, side.h, e.max(), k, frac))
    assert e.max() < ORACLE_VS_F64, (what, e.max(), k)


def test_first_atrous_against_float64(side):
    _, after, _ = side.run("atrous_first")
    ref = denoise_ref.atrous_first(side.planes, side.cam, PHI, DEPTH_THR, LOBE)
    _against_f64(side, after["PING"], ref, "pass 5")
    hist = side.planes["HIST_LEN"][ref[1]]
    assert (hist >= 3).any() and (hist < 3).any()


@pytest.mark.parametrize("step", STEPS)
def test_stepped_atrous_against_float64(side, step):
    for which, src, dst in ((6, "PING", "PONG"), (7, "PONG", "PING"), (10, "PING", "PONG")):
        _, after, _ = side.run("atrous%d_%d" % (which, step))
        ref = denoise_ref.atrous_step(side.planes, side.cam, side.planes[src], step, FRAME_INDEX, PHI, DEPTH_THR, LOBE)
        _against_f64(side, after[dst], ref, "pass %d step %d" % (which, step))
        if which == 10:
            out, wr = denoise_ref.final_output(side.planes, ref[0])
            _against_f64(side, after["OUTPUT"], (out, wr, ref[2]), "pass 10 step %d output" % step)
            np.testing.assert_array_equal(after["OUTPUT"][~wr], side.planes["ILLUM"][~wr])


DENOISER_TUNING = [dict(firefly_fused=0), dict(ta_supertiles=0), dict(hf_split=1), dict(stencil_tile=32)]


@pytest.mark.parametrize("variant", range(len(DENOISER_TUNING)), ids=lambda v: "-".join(DENOISER_TUNING[v]))
def test_tuning_changes_no_pass_result(side, variant):
    other = Side(side.w, side.h, tuning=DENOISER_TUNING[variant], with_oracle=False)
    try:
        for label, (_, _, written) in SEQUENCE.items():
            _, a, _ = side.run(label)
            _, b, _ = other.run(label)
            for n in written:
                _same_bytes(b[n], a[n], "%s %s %s" % (DENOISER_TUNING[variant], label, n))
    finally:
        other.close()


# [temporal, history fix, clamp, spatial, firefly, a-trous iterations]
SWITCHES = {"temporal_off": [0, 1, 1, 1, 1, 1], "history_fix_off": [1, 0, 1, 1, 1, 1], "clamp_off": [1, 1, 0, 1, 1, 1],
            "spatial_off": [1, 1, 1, 0, 1, 1], "firefly_off": [1, 1, 1, 1, 0, 1], "temporal_alone": [1, 0, 0, 1, 1, 1],
            "temporal_off_spatial_on": [0, 0, 0, 1, 1, 1], "atrous_0": [1, 1, 1, 1, 1, 0], "atrous_2": [1, 1, 1, 1, 1, 2],
            "atrous_3": [1, 1, 1, 1, 1, 3], "all_off": [0, 0, 0, 0, 0, 1],
            "temporal_only": [1, 0, 0, 0, 1, 1], "fix_no_clamp_no_spatial": [1, 1, 0, 0, 1, 1]}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_switch_matrix_on_the_whole_chain(name):
    """The output-source rule (illum / ping / pong / prevIllum), the firefly lists applied by the temporal pass or
    by their own kernel, spatial filtering without stepped passes and with 2 and 3 iterations (steps up to 128 on a
    64-pixel frame): r.denoise against o.denoise, rendered inputs on even frames, synthetic ones on odd frames."""
    w, h = 64, 48
    ints = SWITCHES[name]
    r, o = _setup(w, h)
    try:
        o.set_sky()
        o.set_denoise_params(DN_FLOATS, ints)
        p = vxpt.DenoiseParams(*DN_FLOATS, *ints)
        r.trace(0)
        for f in range(3):
            r.trace(f)  # moves the G-buffer ring like a frame's trace; its planes are overwritten below
            o.trace(f)
            o.post_trace()
            if f % 2:
                planes = denoise_frames.make(w, h, SEED + f, cam=r.camera_info(0))
                for n in denoise_frames.PLANES:
                    o.write(vxpt.BUF[n], planes[n])
            _inject_frame(r, o)
            for n in ("PING", "PONG"):
                r.write(n, o.read(vxpt.BUF[n]))
            r.denoise(f, f + 1, p)
            o.denoise(f, f + 1)
            for n in ("OUTPUT", "PREV_ILLUM", "PREV_FAST"):
                rel = _rel(r.read(n), o.read(vxpt.BUF[n]))
                print(name, f, n, "max rel", rel.max())
                assert rel.max() < RTOL_DN, (name, f, n, rel.max(), np.unravel_index(rel.argmax(), rel.shape))
            np.testing.assert_allclose(r.read("HIST_LEN"), o.read(vxpt.BUF["HIST_LEN"]), rtol=1e-6)
            gres, ores = r.read("RESERVOIRS"), o.read(vxpt.BUF["RESERVOIRS"])
            for fld in RES_FIELDS:
                np.testing.assert_array_equal(gres[fld], ores[fld], err_msg="%s frame %d %s" % (name, f, fld))
            rel = _rel(r.read("ILLUM"), o.read(vxpt.BUF["ILLUM"]))
            assert rel.max() < 1e-5, (name, f, "ILLUM", rel.max())
    finally:
        r.close()


def test_history_saturates_at_the_caps():
    """Three chained frames; the first one's history lengths sit one below, at and one above both caps
    (max_accumulated_frame_num, max_fast_accumulated_frame_num of the parameters in use).  The radiance and
    G-buffer are injected every frame, the histories only before the first."""
    w, h = 37, 29
    r, o = _setup(w, h)
    p = _dn_params()
    cap = p.max_accumulated_frame_num
    try:
        o.set_sky()
        r.trace(0)
        planes = denoise_frames.make(w, h, SEED, params=p, cam=r.camera_info(0))
        assert {cap - 1, cap, cap + 1, p.max_fast_accumulated_frame_num} <= set(planes["PREV_HIST_LEN"].ravel().tolist())
        at_cap = 0
        for f in (1, 2, 3):
            r.trace(f)
            o.trace(f)
            o.post_trace()
            keep = ("PREV_ILLUM", "PREV_FAST", "PREV_HIST_LEN") if f > 1 else ()
            for n in denoise_frames.PLANES:
                if n not in keep:
                    o.write(vxpt.BUF[n], planes[n])
                    r.write(n, planes[n])
            r.denoise(f, f + 1, p)
            o.denoise(f, f + 1)
            gh, oh = r.read("HIST_LEN"), o.read(vxpt.BUF["HIST_LEN"])
            geo = ~planes["_sky"]
            assert gh[geo].max() <= cap
            sat = (oh == cap) & geo
            at_cap += sat.sum()
            np.testing.assert_array_equal(gh[sat], oh[sat])
            np.testing.assert_allclose(gh, oh, rtol=1e-6)
            for n in ("OUTPUT", "PREV_ILLUM", "PREV_FAST"):
                rel = _rel(r.read(n), o.read(vxpt.BUF[n]))
                print("caps frame", f, n, "max rel", rel.max())
                assert rel.max() < RTOL_DN, (f, n, rel.max(), np.unravel_index(rel.argmax(), rel.shape))
        assert at_cap >= 3 * 10
    finally:
        r.close()
