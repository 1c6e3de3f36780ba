"""Float64 numpy evaluation of the render-scale filters, written from their formulas (not from the
library): the 12-tap edge-adaptive upsampler, the 3x3 contrast-adaptive sharpener and the 16-tap
Catmull-Rom resampler.  Images are [h, w, >= 3] arrays; results are [out_h, out_w, 4] float64 with
alpha 0.  Texels outside the image are the edge texels."""
import numpy as np

BICUBIC, EASU, EASU_SHARPEN = 0, 1, 2


def _taps(rgb, ax, ay):
    """tex(dx, dy): the [oh, ow, 3] texels (dx, dy) away from the anchors, edge-clamped."""
    h, w = rgb.shape[:2]

    def tex(dx, dy):
        return rgb[np.clip(ay + dy, 0, h - 1)[:, None], np.clip(ax + dx, 0, w - 1)[None, :]]
    return tex


def easu_anchor(n_in, n_out):
    """texel f of every output column (or row) and the sample position's fraction inside it"""
    s = n_in / n_out
    p = np.arange(n_out, dtype=np.float64) * s + (0.5 * s - 0.5)
    f = np.floor(p)
    return f.astype(np.int64), p - f


def easu(img, ow, oh, return_fallback=False):
    rgb = np.asarray(img, np.float64)[..., :3]
    h, w = rgb.shape[:2]
    ax, px = easu_anchor(w, ow)
    ay, py = easu_anchor(h, oh)
    tex = _taps(rgb, ax, ay)
    px, py = px[None, :], py[:, None]
    #     b c
    #   e f g h
    #   i j k l
    #     n o
    pos = dict(b=(0, -1), c=(1, -1), e=(-1, 0), f=(0, 0), g=(1, 0), h=(2, 0), i=(-1, 1), j=(0, 1), k=(1, 1),
               l=(2, 1), n=(0, 2), o=(1, 2))
    c = {name: tex(*d) for name, d in pos.items()}
    lum = {name: 0.5 * v[..., 0] + v[..., 1] + 0.5 * v[..., 2] for name, v in c.items()}  # by position

    dirx = np.zeros((oh, ow))
    diry = np.zeros((oh, ow))
    length = np.zeros((oh, ow))

    def axis_len(d, m):  # clamp(|d| / m)^2, 0 where the two differences are flat
        safe = np.where(m > 0, m, 1.0)
        return np.where(m > 0, np.clip(np.abs(d) / safe, 0.0, 1.0) ** 2, 0.0)

    # the + pattern (above, left, centre, right, below) around f, g, j, k with its bilinear weight
    for wgt, (A, B, C, D, E) in (((1 - px) * (1 - py), "befgj"), (px * (1 - py), "cfghk"),
                                 ((1 - px) * py, "fijkn"), (px * py, "gjklo")):
        lA, lB, lC, lD, lE = (lum[t] for t in (A, B, C, D, E))
        dx, dy = lD - lB, lE - lA
        dirx += dx * wgt
        diry += dy * wgt
        length += axis_len(dx, np.maximum(np.abs(lD - lC), np.abs(lC - lB))) * wgt
        length += axis_len(dy, np.maximum(np.abs(lE - lC), np.abs(lC - lA))) * wgt

    r2 = dirx * dirx + diry * diry
    zro = r2 < 1.0 / 32768.0
    inv = np.where(zro, 1.0, 1.0 / np.sqrt(np.where(zro, 1.0, r2)))
    dirx = np.where(zro, 1.0, dirx) * inv
    diry = diry * inv
    length = (length * 0.5) ** 2
    stretch = (dirx * dirx + diry * diry) / np.maximum(np.abs(dirx), np.abs(diry))
    len2x = 1.0 + (stretch - 1.0) * length
    len2y = 1.0 - 0.5 * length
    lob = 0.5 + ((1.0 / 4.0 - 0.04) - 0.5) * length
    clp = 1.0 / lob

    acc = np.zeros((oh, ow, 3))
    wsum = np.zeros((oh, ow))
    for name, (dx, dy) in pos.items():
        offx, offy = dx - px, dy - py
        vx = (offx * dirx + offy * diry) * len2x
        vy = (offx * -diry + offy * dirx) * len2y
        d2 = np.minimum(vx * vx + vy * vy, clp)
        wt = (25.0 / 16.0 * (2.0 / 5.0 * d2 - 1.0) ** 2 - 9.0 / 16.0) * (lob * d2 - 1.0) ** 2
        acc += c[name] * wt[..., None]
        wsum += wt
    safe = np.where(wsum != 0, wsum, 1.0)
    res = np.where((wsum != 0)[..., None], acc / safe[..., None], c["f"])
    quad = np.stack([c["f"], c["g"], c["j"], c["k"]])
    res = np.minimum(quad.max(axis=0), np.maximum(quad.min(axis=0), res))
    out = np.concatenate([res, np.zeros((oh, ow, 1))], axis=-1)
    return (out, zro) if return_fallback else out


def sharpen(img, sharpness):
    rgb = np.asarray(img, np.float64)[..., :3]
    h, w = rgb.shape[:2]
    tex = _taps(rgb, np.arange(w), np.arange(h))
    c, west, east, north, south = tex(0, 0), tex(-1, 0), tex(1, 0), tex(0, -1), tex(0, 1)
    plus = np.stack([c, west, east, north, south])
    diag = np.stack([tex(-1, -1), tex(1, -1), tex(-1, 1), tex(1, 1)])
    hi_p, lo_p = plus.max(axis=0), plus.min(axis=0)
    hi_a, lo_a = np.maximum(hi_p, diag.max(axis=0)), np.minimum(lo_p, diag.min(axis=0))
    softmax, softmin = hi_p + hi_a, lo_p + lo_a
    live = (softmax > 0) & (lo_a != hi_a)  # a channel with softmax <= 0, or a flat 3x3, keeps its centre
    safe = np.where(live, softmax, 1.0)
    amp = np.clip(np.minimum(softmin, 2.0 - softmax) / safe, 0.0, 1.0)
    wt = -np.sqrt(amp) / (8.0 - 3.0 * sharpness)
    res = np.where(live, ((north + south + east + west) * wt + c) / (1.0 + 4.0 * wt), c)
    return np.concatenate([res, np.zeros((h, w, 1))], axis=-1)


def bicubic(img, ow, oh):
    rgb = np.asarray(img, np.float64)[..., :3]
    h, w = rgb.shape[:2]

    def axis(n_in, n_out):
        uv = (np.arange(n_out, dtype=np.float64) + 0.5) / n_out * n_in
        f0 = np.floor(uv - 0.5)
        f = uv - (f0 + 0.5)
        f2, f3 = f * f, f * f * f
        w0 = f2 - 0.5 * (f3 + f)
        w1 = 1.5 * f3 - 2.5 * f2 + 1.0
        w3 = 0.5 * (f3 - f2)
        return f0.astype(np.int64), [w0, w1, 1.0 - w0 - w1 - w3, w3]

    ax, wx = axis(w, ow)
    ay, wy = axis(h, oh)
    tex = _taps(rgb, ax, ay)
    acc = np.zeros((oh, ow, 3))
    wsum = np.zeros((oh, ow))
    for j in range(4):
        for i in range(4):
            wt = wy[j][:, None] * wx[i][None, :]
            acc += tex(i - 1, j - 1) * wt[..., None]
            wsum += wt
    return np.concatenate([acc / wsum[..., None], np.zeros((oh, ow, 1))], axis=-1)


def upscale(img, ow, oh, mode, sharpness=1.0):
    if mode == BICUBIC:
        return bicubic(img, ow, oh)
    up = easu(img, ow, oh)
    return sharpen(up, sharpness) if mode == EASU_SHARPEN else up


# ---- the test images (fixed seeds), [h, w, 4] float32 with an arbitrary alpha the filters ignore
def noise_image(w, h, seed=0):
    return np.random.default_rng(seed).random((h, w, 4), dtype=np.float32)


def smooth_image(w, h):
    """Two oblique tanh edges over half a period of a sinusoid and a ramp, inside [0, 1].  Every term
    grows with x and with y, so the luminance gradient vanishes nowhere (the upsampler's
    zero-gradient fallback does not fire: test_easu_is_transposition_equivariant checks it)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    e1 = np.tanh((0.8 * x + 0.6 * y - 0.55 * (0.8 * w + 0.6 * h)) / 1.5)
    e2 = np.tanh((0.5 * x + 0.866 * y - 0.4 * (0.5 * w + 0.866 * h)) / 2.0)
    s = np.sin(np.pi * (0.6 * x / w + 0.4 * y / h) - 0.5 * np.pi)
    ramp = 0.5 * (x / w + y / h)
    img = np.stack([0.35 + 0.15 * e1 + 0.05 * s + 0.30 * ramp,
                    0.35 + 0.12 * e2 + 0.08 * e1 + 0.30 * ramp,
                    0.35 + 0.10 * e1 + 0.10 * e2 + 0.04 * s + 0.30 * ramp,
                    np.full_like(x, 0.5)], axis=-1)
    assert img.min() >= 0.0 and img.max() <= 1.0
    return img.astype(np.float32)


# input (w, h) -> output (w, h): uneven ratio, 1.5, 2, 1, and a footprint wider than the image
SHAPES = [((37, 23), (64, 40)), ((50, 29), (75, 44)), ((24, 16), (48, 32)), ((33, 17), (33, 17)), ((5, 3), (16, 16))]
MODES = [BICUBIC, EASU, EASU_SHARPEN]
BAR = 2e-4  # the project's post-process bar (max abs error against the float64 evaluation)
