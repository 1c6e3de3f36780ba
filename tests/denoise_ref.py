"""Test helper (numpy, no GPU): the denoiser's spatial filter evaluated in float64, restated from the
reference's sources -- not from denoise.hip or the oracle's orc_denoise.cpp.

  atrous_first   AtrousSmem<8, 2> (AtrousSmem.h:66-303): PrevIllumination -> IlluminationPing
                 (Denoiser.cu:250-261), both branches of the history test (:155)
  atrous_step    Atrous (Atrous.h:6-159) at any step, with the hashed offset of steps above 4 (:76-84)
  final_output   the final pass's remodulated output: filtered rgb x albedo, alpha 0, sky pixels left alone
                 (Denoiser.cu:362-392)

The reference's Float4 operators are part of what it computes (LinearMath.h:866-874, 925-940): the
binary Float4 + - * / (by a Float4 or a float on the right) return w = z op v.z, and the compound
*= and /= by a float add the scalar to w; float * Float4 and += / /= by a Float4 are componentwise.
So Atrous writes the filtered blue channel into the variance channel (its Float4 products and the final
quotient, Atrous.h:70,139,149), computeVariance blurs the blue channel as the second moment
(AtrousSmem.h:32), and `sum /= sumW` (:235) leaves w = sum of w x second moment + sumW.

Radiance, weights and positions are float64 (fp32 inputs and fp32 literals taken as exact values).
What selects a texel or a branch by an integer is evaluated exactly as the reference's fp32 /
integer operations: clamped coordinates, the 16-bit material read, the hash, the truncated offset,
the float equality of material ids and the history test on the stored fp32 history length.

Each filter returns (out, written, ambiguous): `out` float64 (H, W, 4), valid where `written` (the
pixels inside the denoising range; the others keep what the plane held); `ambiguous` marks pixels one
of whose taps sits within a relative AMBIGUOUS_REL of a hard threshold, where an fp32 evaluation may
legitimately take the other side:
  * the tap cut-off `weight > 1e-4f` (Atrous.h:129): |weight / 1e-4 - 1| < AMBIGUOUS_REL;
  * `sampleViewZ < 500000` (Atrous.h:120) and the centre's early-out (:44, AtrousSmem.h:137):
    |z / 500000 - 1| < AMBIGUOUS_REL;
  * the plane-distance test (DenoiserCommon.h:293-298): |distance - threshold| < AMBIGUOUS_REL x the
    largest coordinate of the two world positions -- the distance is a difference of positions of that
    size, so an fp32 evaluation carries an absolute error of that order whatever the threshold is.
"""
import numpy as np

AMBIGUOUS_REL = 1e-5
RANGE = 500000.0  # Atrous.h:44,120, AtrousSmem.h:137
LUMA = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], np.float64)  # LinearMath.h:1582-1586
K3 = np.array([np.float32(0.44198), np.float32(0.27901)], np.float64)  # Atrous.h:72, AtrousSmem.h:181


def f32(v):
    return float(np.float32(v))


def _lum(rgb):
    return rgb[..., :3] @ LUMA


def _saturate(x):
    return np.clip(x, 0.0, 1.0)


def _world_pos(cam, xs, ys, depth):
    """GetCurrentWorldPosFromPixelPos (DenoiserCommon.h:272-279) with Camera::uvToWorldDirection
    (Camera.h:102-107); cam = the 32 floats of vxpt_get_camera"""
    cam = np.asarray(cam, np.float64)
    u = (xs.astype(np.float64) + 0.5) * cam[26]
    v = (ys.astype(np.float64) + 0.5) * cam[27]
    d = cam[6:9] * u[..., None] + cam[9:12] * v[..., None] + cam[12:15]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return cam[0:3] + d * depth[..., None]


def _normal_weight_param(fraction):
    """GetNormalWeightParam2(1, fraction) (DenoiserCommon.h:366-382)"""
    p = _saturate(fraction)
    angle = np.arctan(p / (1.0 - p + f32(1e-6)))
    return 1.0 / np.maximum(angle, f32(1e-6))


def _normal_weight(cn, sn, nwp):
    """ComputeNonExponentialWeight(AcosApprox(dot), nwp, 0) (DenoiserCommon.h:6-15, 33-36, 351-354)"""
    ang = np.sqrt(2.0) * np.sqrt(_saturate(1.0 - (cn * sn).sum(-1)))
    t = _saturate((np.abs(ang * nwp) - 1.0) / (0.0 - 1.0))
    return t * t * (3.0 - 2.0 * t)


def _plane(cwp, cn, swp, thr):
    """GetPlaneDistanceWeight_Atrous (DenoiserCommon.h:293-298) -> (weight, ambiguous)"""
    dist = np.abs(((swp - cwp) * cn).sum(-1))
    scale = np.maximum(np.abs(swp).max(-1), np.abs(cwp).max(-1))
    return (dist < thr).astype(np.float64), np.abs(dist - thr) < AMBIGUOUS_REL * scale


def _ushort(material, xs, ys):
    """Load2DUshort1 on the R32F material surface (Atrous.h:47,110): 16 bits at byte 2x of the row, byte
    coordinate clamped to the row, row clamped to the frame"""
    h, w = material.shape
    bx = np.clip(2 * xs.astype(np.int64), 0, 4 * w - 2)
    bits = np.ascontiguousarray(material).view(np.uint32)[np.clip(ys, 0, h - 1), bx >> 2]
    return np.where((bx >> 1) & 1, bits >> 16, bits) & 0xFFFF


def _hash(x):
    """SequenceHash (DenoiserCommon.h:407-427) on uint32 arrays"""
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def _explode(x):
    x = x.astype(np.uint64)
    for s, k in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        x = (x | (x << np.uint64(s))) & np.uint64(k)
    return x


def hashed_offset(xs, ys, frame_index, step):
    """Atrous.h:76-84: Int2(Float2(step) * 0.5f * (RngHashGetFloat2 - 0.5f)), in fp32 and truncated as the
    reference does (DenoiserCommon.h:429-506)"""
    if step <= 4:
        return np.zeros_like(xs), np.zeros_like(ys)
    m = np.uint64(0xFFFFFFFF)
    lin = _explode(xs) | (_explode(ys) << np.uint64(1))
    seed = _hash(np.uint64((frame_index + 0x035F9F29) & 0xFFFFFFFF) + np.zeros_like(lin))
    st = seed ^ ((_hash(lin) + np.uint64(0x9E3779B9) + ((seed << np.uint64(6)) & m) + (seed >> np.uint64(2))) & m)
    u0 = _hash(st)
    u1 = _hash(u0)
    half = np.float32(step) * np.float32(0.5)
    off = []
    for u in (u0, u1):
        r = u.astype(np.uint32).astype(np.float32) / np.float32(4294967295.0)
        off.append(np.trunc(half * (r - np.float32(0.5))).astype(np.int64))
    return off[0], off[1]


def atrous_first(planes, cam, phi_luminance, depth_threshold, lobe_angle_fraction):
    depth = planes["DEPTH"].astype(np.float64)
    h, w = depth.shape
    nr = planes["NORMAL_ROUGH"].astype(np.float64)[..., :3]
    mat = planes["MATERIAL"]
    src = planes["PREV_ILLUM"].astype(np.float64)
    hist = planes["HIST_LEN"]
    ys, xs = np.mgrid[0:h, 0:w]
    # Preload (AtrousSmem.h:41-64): every tap is the clamped pixel's record, its world position included
    wp = _world_pos(cam, xs, ys, depth)

    def tap(a, dx, dy):
        return a[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]

    nwp = _normal_weight_param(f32(lobe_angle_fraction))
    written = ~(planes["DEPTH"] > np.float32(RANGE))
    ambiguous = np.abs(depth / RANGE - 1.0) < AMBIGUOUS_REL

    # history >= 3 (:155-249)
    vs = np.zeros((h, w, 4))
    kern = [1.0 / 4.0, 1.0 / 8.0, 1.0 / 8.0, 1.0 / 16.0]
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            t = tap(src, dx, dy) * kern[abs(dx) * 2 + abs(dy)]  # Float4 * float: w = z * k
            t[..., 3] = t[..., 2]
            vs += t
    var = np.maximum(0.0, vs[..., 3] - _lum(vs) ** 2)
    phi_inv = 1.0 / np.maximum(f32(1e-4), f32(phi_luminance) * np.sqrt(var))
    c_lum = _lum(src)
    thr = f32(depth_threshold) * depth
    sum_w, acc = np.zeros((h, w)), np.zeros((h, w, 4))
    amb3 = np.zeros((h, w), bool)
    for cx in (-1, 0, 1):
        for cy in (-1, 0, 1):
            inside = (xs + cx >= 0) & (ys + cy >= 0) & (xs + cx < w) & (ys + cy < h)
            kernel = np.where(inside, K3[abs(cx)] * K3[abs(cy)], 0.0)
            si = tap(src, cx, cy)
            if cx == 0 and cy == 0:
                wgt = kernel
            else:
                geo, amb = _plane(wp, nr, tap(wp, cx, cy), thr)
                eq = tap(mat, cx, cy) == mat
                amb3 |= amb & inside & eq
                wgt = geo * kernel * _normal_weight(nr, tap(nr, cx, cy), nwp) * \
                    np.exp(-np.abs(c_lum - _lum(si)) * phi_inv) * eq
            sum_w += wgt
            acc += wgt[..., None] * si
    sum_w = np.maximum(sum_w, f32(1e-6))
    acc[..., :3] /= sum_w[..., None]
    acc[..., 3] += sum_w  # Float4 /= float: w += a
    out3 = np.concatenate([acc[..., :3], np.maximum(0.0, acc[..., 3] - _lum(acc) ** 2)[..., None]], -1)

    # history < 3 (:250-302): 5x5, the normal weight alone, variance boosted
    sw, si3, s1, s2 = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    for cx in range(-2, 3):
        for cy in range(-2, 3):
            smp = tap(src, cx, cy)
            wgt = _normal_weight(nr, tap(nr, cx, cy), nwp) * (tap(mat, cx, cy) == mat)
            sw += wgt
            si3 += smp[..., :3] * wgt[..., None]
            s1 += _lum(smp) * wgt
            s2 += smp[..., 3] * wgt
    boost = np.maximum(1.0, 4.0 / (hist.astype(np.float64) + 1.0))
    sw = np.maximum(sw, f32(1e-6))
    si3, s1, s2 = si3 / sw[..., None], s1 / sw, s2 / sw
    out5 = np.concatenate([si3, (np.maximum(0.0, s2 - s1 * s1) * boost)[..., None]], -1)

    wide = hist >= np.float32(3.0)  # the fp32 history length against (float)3u (:150-155)
    out = np.where(wide[..., None], out3, out5)
    return out, written, (ambiguous | (amb3 & wide)) & written


def atrous_step(planes, cam, src, step, frame_index, phi_luminance, depth_threshold, lobe_angle_fraction, cut=1e-4):
    """src: the (H, W, 4) input plane (rgb + variance); cut: the tap cut-off (Atrous.h:129; another value only to
    show that a frame holds taps near it)"""
    depth32 = planes["DEPTH"]
    depth = depth32.astype(np.float64)
    h, w = depth.shape
    nr = planes["NORMAL_ROUGH"].astype(np.float64)[..., :3]
    mat = planes["MATERIAL"]
    hist = planes["HIST_LEN"].astype(np.float64)
    src = src.astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    written = ~(depth32 > np.float32(RANGE))
    ambiguous = np.abs(depth / RANGE - 1.0) < AMBIGUOUS_REL
    c_mat = _ushort(mat, xs, ys)
    cwp = _world_pos(cam, xs, ys, depth)
    lobe = f32(lobe_angle_fraction) / np.sqrt(float(step))
    lobe = f32(0.99) + (lobe - f32(0.99)) * _saturate(hist / 5.0)  # lerp (:59)
    nwp = _normal_weight_param(lobe)
    c_lum = _lum(src)
    phi_inv = 1.0 / np.maximum(f32(1e-4), f32(phi_luminance) * np.sqrt(src[..., 3]))
    kc = K3[0] * K3[0]
    sum_w = np.full((h, w), kc)
    acc = src * kc
    acc[..., 3] = acc[..., 2]  # Float4 * Float4: w = z * v.z
    thr = f32(depth_threshold) * depth
    ox, oy = hashed_offset(xs, ys, frame_index, step)
    cut = f32(cut)
    for yy in (-1, 0, 1):
        for xx in (-1, 0, 1):
            if xx == 0 and yy == 0:
                continue
            px, py = xs + ox + xx * step, ys + oy + yy * step
            inside = (px >= 0) & (py >= 0) & (px < w) & (py < h)
            cpx, cpy = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
            sz = depth[cpy, cpx]
            swp = _world_pos(cam, px, py, sz)  # the unclamped pixel's ray, the clamped texel's depth (:114-115)
            geo, amb_p = _plane(cwp, nr, swp, thr)
            near = inside & (sz < RANGE)
            amb_z = inside & (np.abs(sz / RANGE - 1.0) < AMBIGUOUS_REL)
            eq = _ushort(mat, px, py) == c_mat
            wgt = geo * K3[abs(xx)] * K3[abs(yy)] * near * _normal_weight(nr, nr[cpy, cpx], nwp) * eq
            # the weight the other side of the plane test would give decides whether the test matters
            alt = K3[abs(xx)] * K3[abs(yy)] * near * _normal_weight(nr, nr[cpy, cpx], nwp) * eq
            ambiguous |= (amb_p & (alt > 0.5 * cut)) | (amb_z & eq) | (np.abs(wgt / cut - 1.0) < AMBIGUOUS_REL)
            take = wgt > cut
            sv = src[cpy, cpx]
            wgt = np.where(take, wgt * np.exp(-np.abs(c_lum - _lum(sv)) * phi_inv), 0.0)
            sum_w += wgt
            acc += wgt[..., None] * sv[..., [0, 1, 2, 2]]  # Float4 * Float4, then a componentwise +=
    out = acc / sum_w[..., None]
    out[..., 3] = out[..., 2]  # Float4 / Float4: w = z / v.z
    return out, written, ambiguous & written


def final_output(planes, filtered):
    """rgb x albedo, alpha 0, on the pixels inside the denoising range (the others keep the sky copy)"""
    out = np.zeros(filtered.shape)
    out[..., :3] = filtered[..., :3] * planes["ALBEDO"].astype(np.float64)[..., :3]
    return out, ~(planes["DEPTH"] > np.float32(RANGE))
