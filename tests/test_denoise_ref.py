"""The oracle's spatial filter (oracle/orc_denoise.cpp, fp32) against its float64 restatement
(tests/denoise_ref.py) on the synthetic edge frames of tests/denoise_frames.py, and the builder's
self-check.  CPU only.

Measured: the oracle's largest relative error (`_rel` of test_gpu_parity, floor 1e-3) against float64 over
every case below, non-ambiguous pixels, is 5.3e-6 (pass 5 at 17x33; the stepped passes and the final output
stay below 7e-7: MEASURED); the bar ORACLE_VS_F64 = 1e-5 is that value rounded up to the next power of ten,
below RTOL_DN = 1e-4.  Ambiguous pixels: at most 0.39 % of the geometry (2 pixels of 17x33, pass 5).  tests/test_gpu_denoise_stages.py holds the GPU kernels to the same bar.
"""
import numpy as np
import pytest

import denoise_frames
import denoise_ref
import oracle
import vxpt
from golden.make_golden import C1_CAMERA
from test_gpu_parity import DN_FLOATS, DN_INTS, RTOL_DN, _rel

# oracle vs float64, max _rel per pass over the four sizes (non-ambiguous pixels)
MEASURED = {"pass5": 5.3e-6, "step2": 3.0e-7, "step4": 3.0e-7, "step8": 6.4e-7, "step16": 2.7e-7, "step32": 4.1e-7,
            "final": 3.1e-7}
ORACLE_VS_F64 = 1e-5  # 5.3e-6 (pass 5: small normal weights, 1 - dot and the smoothstep's tail amplify fp32 rounding) rounded up
AMBIGUOUS_CAP = 0.005
SEED = 5
FRAME_INDEX = 3
PHI, DEPTH_THR, LOBE = DN_FLOATS[2], DN_FLOATS[5], DN_FLOATS[3]
# (oracle pass, step, source plane, destination plane)
STEPS = [(6, 2, "PING", "PONG"), (7, 4, "PONG", "PING"), (6, 8, "PING", "PONG"), (7, 16, "PONG", "PING"),
         (6, 32, "PING", "PONG")]


def make_oracle(w, h):
    o = oracle.Oracle(w, h)
    o.set_camera(C1_CAMERA[0], C1_CAMERA[1], fov=C1_CAMERA[2])
    o.set_camera(C1_CAMERA[0], C1_CAMERA[1], fov=C1_CAMERA[2], which=1)
    o.set_denoise_params(DN_FLOATS, DN_INTS)
    return o


_CASES = {}


def case(w, h):
    """The frame, an oracle holding it and the float64 results, computed once per size and left unchanged."""
    if (w, h) not in _CASES:
        o = make_oracle(w, h)
        planes = denoise_frames.make(w, h, SEED, cam=o.camera_info(0))
        cam = o.camera_info(0)
        ref = {"pass5": denoise_ref.atrous_first(planes, cam, PHI, DEPTH_THR, LOBE)}
        for _, step, src, _ in STEPS:
            ref["step%d" % step] = denoise_ref.atrous_step(planes, cam, planes[src], step, FRAME_INDEX, PHI, DEPTH_THR, LOBE)
        ref["step64"] = denoise_ref.atrous_step(planes, cam, planes["PING"], 64, FRAME_INDEX, PHI, DEPTH_THR, LOBE)
        _CASES[(w, h)] = (planes, o, cam, ref)
    return _CASES[(w, h)]


def check_against_ref(got, ref, planes, what, bar):
    """got: fp32 plane; ref = (out, written, ambiguous).  Returns the largest error on the compared pixels."""
    out, written, amb = ref
    geo = ~planes["_sky"]
    frac = amb[geo].mean()
    assert frac <= AMBIGUOUS_CAP, (what, "ambiguous fraction", frac)
    use = written & ~amb
    e = _rel(got.astype(np.float64), out)[use]
    k = np.argwhere(use)[e.max(-1).argmax()] if e.size else None
    print("%s: max rel %.3e at (y, x) %s, ambiguous %.4f" % (what, e.max(), k, frac))
    assert e.max() < bar, (what, e.max(), k)
    return float(e.max())


@pytest.mark.parametrize("w,h", denoise_frames.SIZES)
def test_oracle_first_atrous_against_float64(w, h):
    planes, o, cam, ref = case(w, h)
    denoise_frames.write_planes(o, planes, vxpt.BUF)
    o.run_pass(5)
    got = o.read(vxpt.BUF["PING"])
    check_against_ref(got, ref["pass5"], planes, "pass 5 %dx%d" % (w, h), ORACLE_VS_F64)
    keep = ~ref["pass5"][1]
    np.testing.assert_array_equal(got[keep], planes["PING"][keep])
    # both branches ran
    hist = planes["HIST_LEN"][ref["pass5"][1]]
    assert (hist >= 3).any() and (hist < 3).any()


@pytest.mark.parametrize("w,h", denoise_frames.SIZES)
@pytest.mark.parametrize("k", range(len(STEPS)))
def test_oracle_stepped_atrous_against_float64(w, h, k):
    planes, o, cam, ref = case(w, h)
    which, step, src, dst = STEPS[k]
    denoise_frames.write_planes(o, planes, vxpt.BUF)
    o.run_pass(which, step, FRAME_INDEX)
    got = o.read(vxpt.BUF[dst])
    r = ref["step%d" % step]
    check_against_ref(got, r, planes, "step %d %dx%d" % (step, w, h), ORACLE_VS_F64)
    np.testing.assert_array_equal(got[~r[1]], planes[dst][~r[1]])
    np.testing.assert_array_equal(o.read(vxpt.BUF[src]), planes[src])


@pytest.mark.parametrize("w,h", denoise_frames.SIZES)
def test_oracle_final_output_against_float64(w, h):
    """pass 6 at step 2 followed by the remodulated copy (oracle pass 8 from PONG): the final output"""
    planes, o, cam, ref = case(w, h)
    denoise_frames.write_planes(o, planes, vxpt.BUF)
    o.run_pass(6, 2, FRAME_INDEX)
    o.run_pass(1)
    o.run_pass(8, vxpt.BUF["PONG"])
    flt, written, amb = ref["step2"]
    out, wr = denoise_ref.final_output(planes, flt)
    got = o.read(vxpt.BUF["OUTPUT"])
    check_against_ref(got, (out, wr, amb), planes, "final %dx%d" % (w, h), ORACLE_VS_F64)
    np.testing.assert_array_equal(got[~wr], planes["ILLUM"][~wr])  # sky pixels: the radiance as it is


def test_measured_bar_is_the_rounded_maximum():
    worst = max(MEASURED.values())
    assert ORACLE_VS_F64 == 10.0 ** np.ceil(np.log10(worst))
    assert ORACLE_VS_F64 <= RTOL_DN


def test_sky_depth_is_what_the_trace_writes():
    o = make_oracle(32, 24)
    o.terrain((2, 1, 2))
    o.set_sky()
    o.trace(0, primary_only=True)
    d = o.read(vxpt.BUF["DEPTH"])
    assert (d > 5e5).any() and (d[d > 5e5] == denoise_frames.SKY_DEPTH).all()


@pytest.mark.parametrize("w,h", denoise_frames.SIZES)
def test_builder_holds_every_edge(w, h):
    planes, o, cam, _ = case(w, h)
    sky = planes["DEPTH"] > 5e5
    geo = ~sky
    np.testing.assert_array_equal(sky, planes["_sky"])
    for name in denoise_frames.PLANES:
        if name != "RESERVOIRS":
            assert planes[name].dtype == np.float32 and np.isfinite(planes[name]).all(), name

    def ring(mask, y, x):
        blk = mask[y - 1:y + 2, x - 1:x + 2].copy()
        blk[1, 1] = not mask[y, x]
        return blk

    # depth: isolated pixels, corners, sky block, a discontinuity between the two planes
    y, x = planes["_sky_in_geo"]
    assert sky[y, x] and ring(geo, y, x).all()
    y, x = planes["_geo_in_sky"]
    assert geo[y, x] and ring(sky, y, x).all()
    assert geo[0, 0] and geo[0, w - 1] and geo[h - 1, 0] and geo[h - 1, w - 1]
    assert (planes["DEPTH"][sky] == denoise_frames.SKY_DEPTH).all() and sky.sum() >= 9
    d = planes["DEPTH"].astype(np.float64)
    jump = (np.abs(np.diff(d, axis=1)) > 0.1 * d[:, 1:]) & geo[:, 1:] & geo[:, :-1]
    assert jump.sum() >= 3
    # normals: unit or zero; axis-aligned and oblique; a change inside a 3x3 window; zero normals
    n = planes["NORMAL_ROUGH"][..., :3].astype(np.float64)
    ln = np.linalg.norm(n, axis=-1)
    assert set(map(tuple, np.argwhere(ln == 0))) == set(planes["_zero_normals"]) and len(planes["_zero_normals"]) == 3
    assert np.allclose(ln[ln > 0], 1.0, atol=1e-6)
    axis = (np.abs(n).max(-1) == 1.0)
    assert axis.any() and ((ln > 0) & ~axis).any()
    assert ((n[1:, 1:] != n[:-1, :-1]).any(-1) & (ln[1:, 1:] > 0) & (ln[:-1, :-1] > 0)).sum() >= 4
    rough = planes["NORMAL_ROUGH"][..., 3]
    assert (rough == 0).any() and (rough == 1).any() and ((rough > 0) & (rough < 1)).any()
    # material: id 0, the largest 16-bit id, stencils that straddle a change (3x3, 5x5 and stepped)
    m = planes["MATERIAL"]
    ys, xs = np.mgrid[0:h, 0:w]
    us = denoise_ref._ushort(m, xs, ys)
    assert (m == 0).any() and (us == 0).any() and (us == 0xFFFF).any()
    assert (m[:, 1:] != m[:, :-1]).sum() >= h * 3 and (m[:, 2:] != m[:, :-2]).any()
    for step in (2, 4, 8):
        assert (denoise_ref._ushort(m, xs + step, ys) != us).any() and (denoise_ref._ushort(m, xs + step, ys) == us).any()
    # taps between the stepped passes' cut-off and ten times it: a cut-off of 1e-3 would change the result
    moved = 0
    for step in (2, 4, 8):
        a = denoise_ref.atrous_step(planes, cam, planes["PING"], step, FRAME_INDEX, PHI, DEPTH_THR, LOBE)
        b = denoise_ref.atrous_step(planes, cam, planes["PING"], step, FRAME_INDEX, PHI, DEPTH_THR, LOBE, cut=1e-3)
        moved += ((_rel(a[0], b[0]).max(-1) > 2 * RTOL_DN) & a[1] & ~a[2] & ~b[2]).sum()
    print("pixels a cut-off of 1e-3 moves by more than 2e-4:", moved)
    assert moved >= 2, moved
    # history: every listed value on geometry, in both planes
    for name in ("HIST_LEN", "PREV_HIST_LEN"):
        for v in denoise_frames.history_values(DN_FLOATS[0], DN_FLOATS[1]):
            assert ((planes[name] == v) & geo).sum() >= 1, (name, v)
    for cap in (DN_FLOATS[0], DN_FLOATS[1]):
        assert {cap - 1, cap, cap + 1} <= set(planes["_history_values"].tolist())
    # radiance patches in all five planes
    p = planes["_patches"]
    plain = np.ones((h, w), bool)
    for (y, x) in planes["_outliers"]:  # their radiance is scaled
        plain[y, x] = False
    for name in ("ILLUM", "PREV_ILLUM", "PREV_FAST", "PING", "PONG"):
        a = planes[name]
        ok = plain if name == "ILLUM" else np.ones((h, w), bool)
        assert (a[p["zero"]][..., :3 if name == "ILLUM" else 4] == 0).all()
        for key, val in (("big", 1e4), ("tiny", 1e-6)):
            assert (a[p[key]][..., :3][ok[p[key]]] == np.float32(val)).all(), (name, key)
        c = a[p["const"]][..., :3][ok[p["const"]]]
        assert len(c) >= 9 and (c == c[0]).all(), name
    assert (planes["PING"][p["const"]][..., 3] == 0).all() and (planes["PING"][p["big"]][..., 3] == np.float32(1e8)).all()
    # motion: zero, sub-pixel, onto the frame edge, out of the frame (previous pixel column)
    mv = planes["MOTION"][..., :3].astype(np.float64)
    assert (np.abs(mv).sum(-1) == 0).any() and planes["_subpixel"].any()
    wp = denoise_ref._world_pos(cam, xs, ys, d) + mv
    cam64 = np.asarray(cam, np.float64)
    wtu = np.stack([cam64[15:18], cam64[18:21], cam64[21:24]], 1)  # columns
    q = (wp - cam64[0:3]) @ wtu.T
    col = q[..., 0] / q[..., 2] * w
    sub = planes["_subpixel"]
    shift = np.abs(col - (xs + 0.5))[sub]
    assert (shift > 0.05).all() and (shift < 0.95).all()
    cols = np.arange(w // 2, min(w // 2 + 4, w))
    assert np.abs(col[planes["_motion_rows"]["edge"], cols]).max() < 1e-3
    assert (col[planes["_motion_rows"]["out"], cols] < -1.0).all()
    # disocclusion: the temporal pass leaves a dense history-fix list in one tile (where the frame has two)
    # and sparse ones elsewhere
    dis = planes["_disoccluded"]
    assert (planes["PREV_DEPTH"][dis] != planes["DEPTH"][dis]).all() and (planes["PREV_DEPTH"][~dis] == planes["DEPTH"][~dis]).all()
    denoise_frames.write_planes(o, planes, vxpt.BUF)
    o.run_pass(2)
    fix = (o.read(vxpt.BUF["HIST_LEN"]) <= 4) & geo
    dense = sparse = 0
    for ty in range((h + 15) // 16):
        for tx in range((w + 15) // 16):
            ys_, xs_ = slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16)
            nfix, ndis = fix[ys_, xs_].sum(), dis[ys_, xs_].sum()
            if (tx, ty) == planes["_dense_tile"]:
                assert nfix > 64 and ndis == geo[ys_, xs_].sum(), (tx, ty, nfix)
                dense += 1
            else:
                assert ndis <= 5 and nfix <= 64, (tx, ty, nfix, ndis)
                sparse += 1 if 0 < nfix else 0
    assert sparse >= 1 and dense == (1 if w * h > 256 else 0)
    # reservoirs: outliers, the adjacent pair, the tile with a single valid reservoir
    res = planes["RESERVOIRS"][:w * h].reshape(h, w)
    valid = (res["lightData"] != 0) & (res["weightSum"] > 0)
    assert (valid == (geo & valid)).all() and valid[geo].mean() > 0.8
    for (y, x) in planes["_outliers"]:
        assert valid[y, x] and res["weightSum"][y, x] >= 10.0
    (y0, x0), (y1, x1) = planes["_pair"]
    assert y0 == y1 and x1 == x0 + 1 and x0 // 8 != x1 // 8
    y, x = planes["_lonely"]
    assert valid[y // 4 * 4:y // 4 * 4 + 4, x // 8 * 8:x // 8 * 8 + 8].sum() == 1
