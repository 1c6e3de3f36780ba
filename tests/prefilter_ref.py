"""Numpy evaluation of the denoiser's hit-distance reconstruction and pre-pass blur, written from their
formulas (not from the library), plus the synthetic planes the tests run them on.

Weights and sums are float64.  The pre-pass's tap coordinates are float32, in the body's operation order
(hit distance / frustum size -> blur radius -> rotated Poisson offset -> floor): a coordinate is an
integer decision, so it has to round as the body rounds.  prepass() also takes precomputed coordinates.

Planes: illum and normal_rough [h, w, 4], depth and material [h, w].  camera = (pos, dir, fov_deg)."""
import numpy as np

RANGE = 500000.0
F = np.float32


def _c(x):  # a float literal of the kernels, as the float64 value of its float32
    return float(F(x))


POISSON8 = np.array([(-0.4706069, -0.4427112, +0.6461146), (-0.9057375, +0.3003471, +0.9542373),
                     (-0.3487388, +0.4037880, +0.5335386), (+0.1023042, +0.6439373, +0.6520134),
                     (+0.5699277, +0.3513750, +0.6695386), (+0.2939128, -0.1131226, +0.3149309),
                     (+0.7836658, -0.4208784, +0.8895339), (+0.1564120, -0.8198990, +0.8346850)], F)


# ---------------------------------------------------------------- camera (float64)
def camera_basis(camera, w, h):
    """(pos, M): the primary ray of uv is normalize(M @ (u, v, 1))"""
    pos, d, fov = (np.asarray(camera[0], np.float64), np.asarray(camera[1], np.float64), float(camera[2]))
    d = d / np.linalg.norm(d)
    left = np.cross((0.0, 1.0, 0.0), d)
    left /= np.linalg.norm(left)
    up = np.cross(d, left)
    up /= np.linalg.norm(up)
    fov_x = np.radians(fov)
    fov_y = fov_x * (h / w)
    tx, ty = np.tan(fov_x / 2), np.tan(fov_y / 2)
    view_to_world = np.stack([-left, up, d], axis=1)
    m = view_to_world @ np.diag([tx, ty, 1.0]) @ np.array([[2.0, 0, -1], [0, 2.0, -1], [0, 0, 1]])
    return pos, m


def ray_dirs(camera, w, h, xs, ys):
    pos, m = camera_basis(camera, w, h)
    uv1 = np.stack([(xs + 0.5) / w, (ys + 0.5) / h, np.ones_like(xs, np.float64)], axis=-1)
    d = uv1 @ m.T
    return pos, d / np.linalg.norm(d, axis=-1, keepdims=True)


def world_pos(camera, w, h, xs, ys, depth):
    pos, d = ray_dirs(camera, w, h, xs, ys)
    return pos + d * depth[..., None]


# ---------------------------------------------------------------- hit-distance reconstruction
def hitdist(illum, depth, normal_rough):
    il = np.asarray(illum, np.float64)
    h, w = il.shape[:2]
    hd, vz, n = il[..., 3], np.abs(np.asarray(depth, np.float64)), np.asarray(normal_rough, np.float64)[..., :3]
    ys, xs = np.mgrid[0:h, 0:w]
    nwp = 1.0 / np.arctan(0.75 / (1.0 - 0.75))
    sum_w = 1000.0 * (hd != 0.0)
    acc = hd * sum_w
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                continue
            sy, sx = np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)
            inside = (ys + dy >= 0) & (ys + dy < h) & (xs + dx >= 0) & (xs + dx < w)
            cosa = np.clip((n * n[sy, sx]).sum(-1), 0.0, 1.0)
            angle = np.sqrt(2.0) * np.sqrt(np.clip(1.0 - cosa, 0.0, 1.0))
            r = np.hypot(dx, dy) * 0.5
            g = np.exp(-_c(0.66) * r * r)
            sz = vz[sy, sx]
            t = np.abs(sz - vz) / (np.maximum(sz, vz) + _c(1e-6))
            bil = np.clip((t - _c(0.03)) / (0.0 - _c(0.03)), 0.0, 1.0)
            v = -3.0 * np.abs(angle * nwp)
            dw = inside * g * bil / (v * v - v + 1.0)
            shd = np.where(dw == 0.0, 0.0, hd[sy, sx])
            dw = dw * (shd != 0.0)
            acc += shd * dw
            sum_w += dw
    out = il.copy()
    out[..., 3] = np.where(vz > RANGE, hd, acc / np.maximum(sum_w, _c(1e-6)))
    return out


# ---------------------------------------------------------------- pre-pass
def rotator(iteration_index):
    """(cos, sin) of Weyl1D(0.5, n) * 90 degrees, float32"""
    prod = np.array(iteration_index * 10368889, np.int64).astype(np.int32)  # the int product wraps
    v = F(0.5) + F(prod) / F(16777216.0)
    weyl = F(v - np.trunc(v))
    a1 = weyl * F(90.0 * (np.pi / float(F(180.0))))
    return F(np.cos(np.float64(a1))), F(np.sin(np.float64(a1)))


def blur_radius(illum, depth, camera):
    """float32, the body's order: 30 * saturate(hitDist / (min(w, h) * K * z)), >= 1 where hitDist = 0"""
    hd, z = np.asarray(illum, F)[..., 3], np.asarray(depth, F)
    h, w = z.shape
    tan_x = F(np.tan(np.float64(F(camera[2]) * F(0.01745329251) * F(0.5))))
    k = tan_x / (F(w) / F(2))
    frustum = F(min(w, h)) * k * z
    hit = np.where(hd == 0, F(1), hd)
    r = F(30) * np.minimum(np.maximum(hit / frustum, F(0)), F(1))
    return np.where(hd == 0, np.maximum(r, F(1)), r).astype(F)


def prepass_coords(illum, depth, camera, iteration_index):
    """[h, w, 8, 2] texel (x, y) of every pixel's taps, before any screen test"""
    r = blur_radius(illum, depth, camera)
    h, w = r.shape
    ca, sa = rotator(iteration_index)
    ys, xs = np.mgrid[0:h, 0:w]
    ux = (xs.astype(F) + F(0.5)) * (F(1) / F(w)) * F(w)
    uy = (ys.astype(F) + F(0.5)) * (F(1) / F(h)) * F(h)
    out = np.zeros((h, w, 8, 2), np.int32)
    for i in range(8):
        ox, oy = POISSON8[i, 0], POISSON8[i, 1]
        rx = F(ox * ca) + F(oy * sa)
        ry = F(ox * F(-sa)) + F(oy * ca)
        out[:, :, i, 0] = np.floor(ux + F(rx) * r).astype(np.int32)
        out[:, :, i, 1] = np.floor(uy + F(ry) * r).astype(np.int32)
    return out


def prepass(illum, depth, normal_rough, material, camera, iteration_index, coords=None):
    if coords is None:
        coords = prepass_coords(illum, depth, camera, iteration_index)
    il, z = np.asarray(illum, np.float64), np.asarray(depth, np.float64)
    n, mat = np.asarray(normal_rough, np.float64)[..., :3], np.asarray(material, np.float64)
    h, w = z.shape
    ys, xs = np.mgrid[0:h, 0:w]
    cwp = world_pos(camera, w, h, xs.astype(np.float64), ys.astype(np.float64), z)
    tan_half = 0.125 / (1.0 - 0.125 + _c(1e-6))
    nwp = 1.0 / max(np.arctan(tan_half), _c(1e-6))
    a = 1.0 / (_c(0.0005) + (1.0 / 9.0) * (1.0 - _c(0.0005)))
    b = il[..., 3] * a
    wsum = np.ones((h, w))
    acc = il.copy()
    for i in range(8):
        ix, iy = coords[:, :, i, 0].astype(np.int64), coords[:, :, i, 1].astype(np.int64)
        inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
        cx, cy = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
        sz, sm, sn, sv = z[cy, cx], mat[cy, cx], n[cy, cx], il[cy, cx]
        swp = world_pos(camera, w, h, ix.astype(np.float64), iy.astype(np.float64), sz)
        wt = inside * (sz < RANGE) * (sm == mat)
        wt = wt * ~(np.abs(((swp - cwp) * n).sum(-1)) / z > _c(0.003))
        angle = np.sqrt(2.0) * np.sqrt(np.clip(1.0 - (n * sn).sum(-1), 0.0, 1.0))
        t = np.clip((np.abs(angle * nwp) - 1.0) / (0.0 - 1.0), 0.0, 1.0)
        wt = wt * (t * t * (3.0 - 2.0 * t))
        s = np.where((wt == 0.0)[..., None], 0.0, sv)
        v = -3.0 * np.abs(s[..., 3] * a - b)
        wt = wt * (_c(0.2) + (1.0 / (v * v - v + 1.0)) * (1.0 - _c(0.2)))
        wt = wt * np.exp(-_c(0.66) * float(POISSON8[i, 2]) ** 2)
        wsum += wt
        acc[..., :3] += s[..., :3] * wt[..., None]
        acc[..., 3] += s[..., 2] * wt  # Float4 * float takes w from z (LinearMath.h:873)
    out = acc.copy()
    out[..., :3] = acc[..., :3] / wsum[..., None]
    out[..., 3] = acc[..., 3] + wsum  # Float4 /= float adds to w (LinearMath.h:933-940)
    sky = z > RANGE
    out[sky] = il[sky]
    return out


# ---------------------------------------------------------------- synthetic planes
CAMERA = ((0.0, 10.0, 0.0), (0.0, -0.35, 1.0), 90.0)
SHAPES = ((50, 29), (24, 20), (136, 72))
ITERATIONS = (1, 7)


def scene(w, h, seed=None, camera=CAMERA):
    """A floor (two materials in stripes) and an oblique wall of finite height (a third material) that
    meet in an edge crossing the frame at an angle, sky above the wall; normals per plane plus small
    noise, noise radiance, hit distances in (0, 50] with about 10 % exact zeros."""
    rng = np.random.default_rng(w * 1000 + h if seed is None else seed)
    ys, xs = np.mgrid[0:h, 0:w]
    pos, d = ray_dirs(camera, w, h, xs.astype(np.float64), ys.astype(np.float64))
    n_floor = np.array([0.0, 1.0, 0.0])
    n_wall = np.array([-0.45, 0.0, -0.893])
    n_wall /= np.linalg.norm(n_wall)
    p_wall = np.array([0.0, 0.0, 38.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t_floor = (0.0 - pos[1]) / d[..., 1]
        t_wall = ((p_wall - pos) @ n_wall) / (d @ n_wall)
    t_floor = np.where(t_floor > 0, t_floor, np.inf)
    hit_y = pos[1] + d[..., 1] * t_wall
    t_wall = np.where((t_wall > 0) & (hit_y < 16.0), t_wall, np.inf)
    depth = np.minimum(t_floor, t_wall)
    is_wall = t_wall < t_floor
    sky = ~np.isfinite(depth)
    wx = pos[0] + d[..., 0] * np.where(sky, 0.0, depth)
    material = np.where(is_wall, 5.0, np.where(np.floor(wx / 6.0) % 2 == 0, 1.0, 2.0))
    normal = np.where(is_wall[..., None], n_wall, n_floor) + rng.normal(0.0, 1e-3, (h, w, 3))
    nr = np.concatenate([normal, np.full((h, w, 1), 0.8)], -1)
    hd = 50.0 * (1.0 - rng.random((h, w)))
    hd[rng.random((h, w)) < 0.1] = 0.0
    illum = np.concatenate([2.0 * rng.random((h, w, 3)), hd[..., None]], -1)
    depth = np.where(sky, 1e27, depth)
    material = np.where(sky, 0.0, material)
    return dict(illum=illum.astype(F), depth=depth.astype(F), normal_rough=nr.astype(F), material=material.astype(F),
                camera=camera)


def nudge(s, seed):
    """The planes with every hit distance, depth and normal component moved by one fp32 ulp, up or down
    at random.  Exact zeros of the hit distance stay: 0 is the flag `no hit`, not a measurement."""
    rng = np.random.default_rng(seed)

    def ulp(a):
        up = rng.random(a.shape) < 0.5
        return np.where(up, np.nextafter(a, F(np.inf)), np.nextafter(a, F(-np.inf))).astype(F)
    out = dict(s)
    il = s["illum"].copy()
    il[..., 3] = np.where(il[..., 3] == 0, il[..., 3], ulp(il[..., 3]))
    nr = s["normal_rough"].copy()
    nr[..., :3] = ulp(nr[..., :3])
    out.update(illum=il, depth=ulp(s["depth"]), normal_rough=nr)
    return out


def rel_diff(a, b, channels=slice(None)):
    """largest |a - b| / max(|b|, 1e-3) over the channels"""
    a, b = np.asarray(a, np.float64)[..., channels], np.asarray(b, np.float64)[..., channels]
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max())
