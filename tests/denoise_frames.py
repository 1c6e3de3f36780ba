"""Test helper (numpy, seeded, no GPU): synthetic denoiser inputs that hold the values on which the
ReLAX passes branch -- rendered terrain frames hold only a handful of them.

make(w, h, seed) returns the planes `_inject_frame` of tests/test_gpu_parity.py writes plus PING and
PONG, keyed by vxpt.BUF names, every value a finite fp32.  Keys that start with "_" are notes about
the layout (masks and pixel lists) for the self-check of tests/test_denoise_ref.py; they are not
planes.

Layout (fractions of the frame, so that every item exists from 16x16 up):
  depth     two planes in world space met by the C1 camera's rays (one facing the camera: an oblique
            normal in world axes; one axis-aligned), split along the frame's diagonal; a sky block
            near the top (not touching the frame edge, so the four corners are geometry) with one
            geometry pixel inside; one sky pixel inside geometry
  normals   the planes' normals; scattered normals tilted by up to 0.9 rad; a checkerboard of two normals (a change inside every 3x3 window
            there); three zero normals; roughness 0 / between / 1 by thirds of the width
  material  vertical 3-pixel stripes of the float ids 1, 2, 3.0039 (bits 0x4040FFFF: its low half is
            the largest id a 16-bit read returns, 65535), 0 and 3
  history   2x2 blocks cycling through 0..7, the two caps -1 / +0 / +1 and a few values between
            (HIST_LEN); PREV_HIST_LEN the same list in 1x1 blocks shifted by one (so that the history
            fix of a tile without disocclusion keeps a sparse list)
  radiance  smooth noise in [0.05, 0.5]; a constant patch (zero variance), a patch of zeros, a patch
            at 1e4 beside one at 1e-6
  motion    zero; a sub-pixel block; a row segment that reprojects onto the frame's left edge; one
            that leaves the frame.  Disocclusion (PREV_DEPTH = 1.5 x DEPTH): one whole 16x16 tile
            where the frame has more than one tile, and at most 5 scattered pixels in every other
            tile
  reservoirs valid over geometry; outliers as tests/test_gpu_paths.py places them, two at distance 1
            in horizontally adjacent 8x4 tiles, and one 8x4 tile whose only valid reservoir is the
            outlier
"""
import numpy as np

import vxpt

SIZES = [(16, 16), (17, 33), (70, 20), (37, 29)]
# the depth the trace writes for a primary ray that leaves the world (Common.h:27 RayMax; asserted
# against a traced frame in tests/test_denoise_ref.py and tests/test_gpu_denoise_stages.py)
SKY_DEPTH = np.float32(1.0e27)
ID_MAX_USHORT = np.array([0x4040FFFF], np.uint32).view(np.float32)[0]  # finite; low 16 bits 0xFFFF
MATERIAL_IDS = np.array([1.0, 2.0, ID_MAX_USHORT, 0.0, 3.0], np.float32)
PLANES = ("PREV_NORMAL_ROUGH", "PREV_DEPTH", "PREV_MATERIAL", "PREV_ILLUM", "PREV_FAST", "PREV_HIST_LEN",
          "HIST_LEN", "ILLUM", "DEPTH", "NORMAL_ROUGH", "MATERIAL", "ALBEDO", "GEO_NORMAL_THIN", "MAT_PARAM",
          "MOTION", "RESERVOIRS", "PING", "PONG")


def history_values(max_acc, max_fast):
    """The history lengths of the block pattern: every branch value, both caps -1 / 0 / +1."""
    caps = [max_fast - 1, max_fast, max_fast + 1, max_acc - 1, max_acc, max_acc + 1]
    return np.array([0, 1, 2, 3, 4, 5, 6, 7] + caps + [9, 12, 15, 18, 20, 22, 25, 26, 27, 28], np.float32)


def default_camera(w, h):
    """camera_info (32 floats) of the C1 camera at w x h, from the oracle's host code."""
    import oracle
    from golden.make_golden import C1_CAMERA
    o = oracle.Oracle(w, h)
    o.set_camera(C1_CAMERA[0], C1_CAMERA[1], fov=C1_CAMERA[2])
    return o.camera_info(0)


def ray_dirs(cam, xs, ys):
    """float64 unit directions of pixel centres (xs, ys may lie outside the frame)."""
    cam = np.asarray(cam, np.float64)
    u = (np.asarray(xs, np.float64) + 0.5) * cam[26]
    v = (np.asarray(ys, np.float64) + 0.5) * cam[27]
    d = cam[6:9] * u[..., None] + cam[9:12] * v[..., None] + cam[12:15]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def make(w, h, seed, params=None, cam=None):
    from test_gpu_parity import DN_FLOATS
    max_acc, max_fast, lobe_angle_fraction = \
        (params.max_accumulated_frame_num, params.max_fast_accumulated_frame_num, params.lobe_angle_fraction) if params \
        else (DN_FLOATS[0], DN_FLOATS[1], DN_FLOATS[3])
    cam = np.asarray(default_camera(w, h) if cam is None else cam, np.float64)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    pos, cdir = cam[0:3], cam[3:6] / np.linalg.norm(cam[3:6])
    d = ray_dirs(cam, xx, yy)

    # ---- depth and normals
    n_a = -cdir  # oblique in world axes
    ax = int(np.abs(cdir).argmax())
    n_b = np.zeros(3)
    n_b[ax] = -np.sign(cdir[ax])  # axis-aligned
    t_a = 12.0 / -(d @ n_a)
    den_b = -(d @ n_b)
    # where a ray grazes the second plane (tall frames have a wide vertical field of view) the first one stays
    lower = (xx * h + yy * w > 1.2 * w * h) & (den_b > 0.2)
    t_b = 20.0 * abs(cdir[ax]) / np.maximum(den_b, 0.2)
    depth = np.where(lower, t_b, t_a)
    normal = np.where(lower[..., None], n_b, n_a)
    sky = np.zeros((h, w), bool)
    sky_rows, x0, x1 = max(3, h // 5), w // 4, (3 * w) // 4
    sky[1:1 + sky_rows, x0:x1] = True
    geo_in_sky = (2, (x0 + x1) // 2)
    sky[geo_in_sky] = False
    sky_in_geo = (h // 2 + 1, w // 4 + 1)
    sky[sky_in_geo] = True
    depth = np.where(sky, np.float64(SKY_DEPTH), depth)
    # checkerboard of two unit normals over the lower-left block; three zero normals
    tilt = n_a + 0.35 * np.roll(n_a, 1)
    tilt /= np.linalg.norm(tilt)
    cb = (yy >= (3 * h) // 4) & (xx < w // 3) & ((xx + yy) % 2 == 1)
    normal = np.where(cb[..., None], tilt, normal)
    # scattered normals tilted by 0.03 .. 0.9 rad off the first plane's: their neighbours (which keep the plane's
    # normal, so the plane test passes) see every normal weight between 0 and 1, the stepped passes' tap
    # cut-off included
    e1 = np.cross(n_a, np.roll(n_a, 1))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n_a, e1)
    scat = (rng.random((h, w)) < 0.25) & ~lower & ~cb
    ang, az = 0.03 + 0.87 * rng.random((h, w, 1)), 2.0 * np.pi * rng.random((h, w, 1))
    # half of them at the angle whose normal weight, seen from a neighbour of settled history at step 2, puts the
    # tap's weight between the cut-off 1e-4 and 1e-3 (smoothstep at 0.04: 4.7e-3, times the 3x3 kernel's 0.08 .. 0.2)
    lobe = lobe_angle_fraction / np.sqrt(2.0)
    nwp = 1.0 / np.arctan(lobe / (1.0 - lobe + 1e-6))
    ang = np.where(rng.random((h, w, 1)) < 0.5, np.arccos(1.0 - 0.5 * (0.96 / nwp) ** 2), ang)
    normal = np.where(scat[..., None], np.cos(ang) * n_a + np.sin(ang) * (np.cos(az) * e1 + np.sin(az) * e2), normal)
    zero_n = [(h // 2 - 2, w // 2), (h - 2, w - 3), (h // 2 + 3, 2)]
    for p in zero_n:
        normal[p] = 0.0
    rough = np.where(xx < w // 3, 0.0, np.where(xx >= (2 * w) // 3, 1.0, 0.35 + 0.3 * rng.random((h, w))))
    nr = np.concatenate([normal, rough[..., None]], -1).astype(np.float32)
    depth = depth.astype(np.float32)

    material = MATERIAL_IDS[(xx // 3) % len(MATERIAL_IDS)]
    albedo = np.concatenate([0.2 + 0.7 * rng.random((h, w, 3)), np.ones((h, w, 1))], -1).astype(np.float32)
    mat_param = np.zeros((h, w, 4), np.float32)
    mat_param[..., 1] = rough

    # ---- history lengths
    hv = history_values(max_acc, max_fast)
    bw = (w + 1) // 2
    hist = hv[((yy // 2) * bw + xx // 2) % len(hv)]
    prev_hist = hv[(yy * w + xx + 1) % len(hv)]

    # ---- radiance
    def smooth(k):
        base = 0.27 + 0.12 * np.sin(0.9 * xx + k) * np.cos(0.7 * yy - 0.5 * k)
        return np.clip(base[..., None] + 0.1 * (rng.random((h, w, 3)) - 0.5), 0.05, 0.5)

    lum_w = np.array([0.2126, 0.7152, 0.0722], np.float32)
    r0, patches = h // 2, {}
    patches["const"] = (slice(r0, r0 + 5), slice(1, 6))
    patches["zero"] = (slice(r0, r0 + 5), slice(6, 11))
    patches["big"] = (slice(r0 + 5, r0 + 8), slice(1, 5))
    patches["tiny"] = (slice(r0 + 5, r0 + 8), slice(5, 9))
    const_rgb = np.array([0.25, 0.5, 0.125], np.float32)
    const_lum = np.float32(np.dot(const_rgb, lum_w))

    def radiance(k, kind):
        """kind: 'moment' (w = second moment), 'variance' (w = variance) or 'plain' (w = 0 / 1)"""
        rgb = smooth(k).astype(np.float32)
        lum = rgb @ lum_w
        var = (0.01 + 0.02 * rng.random((h, w))).astype(np.float32)
        wch = {"moment": lum * lum + var, "variance": var, "plain": np.zeros((h, w), np.float32)}[kind]
        out = np.concatenate([rgb, wch[..., None]], -1).astype(np.float32)
        out[patches["const"]] = [*const_rgb, const_lum * const_lum if kind == "moment" else 0.0]
        out[patches["zero"]] = 0.0
        out[patches["big"]] = [1e4, 1e4, 1e4, {"moment": 2e8, "variance": 1e8, "plain": 0.0}[kind]]
        out[patches["tiny"]] = [1e-6, 1e-6, 1e-6, {"moment": 2e-12, "variance": 1e-12, "plain": 0.0}[kind]]
        return out

    illum = radiance(0.0, "plain")
    illum[..., 3] = 1.0
    prev_illum, prev_fast = radiance(0.4, "moment"), radiance(0.8, "plain")
    ping, pong = radiance(1.2, "variance"), radiance(1.6, "variance")

    # ---- motion (world space: previous position = current + motion; both cameras are the C1 camera)
    wpos = pos + d * depth.astype(np.float64)[..., None]
    motion = np.zeros((h, w, 4), np.float64)
    sub = (yy >= h // 4 + 2) & (yy < h // 2 - 1) & (xx >= w // 2) & ~sky
    motion[sub, :3] = (pos + ray_dirs(cam, xx[sub] + 0.3, yy[sub]) * depth.astype(np.float64)[sub][:, None]) - wpos[sub]
    row_edge, row_out = h - 4, h - 6
    for row, ucol in ((row_edge, -0.5), (row_out, -0.5 - 0.2 * w)):  # pixel-space column of the previous position
        cols = np.arange(w // 2, min(w // 2 + 4, w))
        tgt = pos + ray_dirs(cam, np.full(len(cols), ucol), np.full(len(cols), row)) * depth[row, cols].astype(np.float64)[:, None]
        motion[row, cols, :3] = tgt - wpos[row, cols]
    motion[sky] = 0.0

    # ---- disocclusion
    dis = np.zeros((h, w), bool)
    tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
    dense_tile = (1, 0) if w >= 32 else ((0, 1) if h > 16 else None)  # (tile x, tile y)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            ys, xs = slice(16 * ty, min(16 * ty + 16, h)), slice(16 * tx, min(16 * tx + 16, w))
            if (tx, ty) == dense_tile:
                dis[ys, xs] = True
                continue
            cand = np.argwhere(~sky[ys, xs])
            for k in rng.choice(len(cand), size=min(3, len(cand)), replace=False):
                dis[16 * ty + cand[k][0], 16 * tx + cand[k][1]] = True
    dis &= ~sky
    prev_depth = np.where(dis, depth * np.float32(1.5), depth).astype(np.float32)

    # ---- reservoirs (two parities with the same layout)
    n = w * h
    res = np.zeros(2 * n, vxpt.RESERVOIR_DTYPE)
    one = np.zeros((h, w), vxpt.RESERVOIR_DTYPE)
    one["lightData"] = rng.integers(1, 1 << 20, (h, w))
    one["uvData"] = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    one["weightSum"] = (0.5 + 1.5 * rng.random((h, w))).astype(np.float32)
    one["targetPdf"] = (0.1 + rng.random((h, w))).astype(np.float32)
    one["M"] = rng.integers(1, 20, (h, w)).astype(np.float32)
    one["lightData"][sky] = 0
    lonely = (1, 2)  # its 8x4 tile (0, 0) keeps no other valid reservoir
    keep = one[lonely].copy()
    one["lightData"][0:4, 0:8] = 0
    one[lonely] = keep
    pair = [(h - 3, 7), (h - 3, 8)]
    outliers = [lonely] + pair + [(6, 12), (h // 2 + 2, w - 2)]
    tile_max = {}
    for (y, x) in outliers:
        blk = one["weightSum"][y // 4 * 4:y // 4 * 4 + 4, x // 8 * 8:x // 8 * 8 + 8]
        tile_max[(y, x)] = blk.max()
    for (y, x) in outliers:
        one["weightSum"][y, x] = max(tile_max[(y, x)] * 1e4, 10.0)
        illum[y, x, :3] *= 50.0
    res[:n], res[n:] = one.reshape(-1), one.reshape(-1)

    out = dict(PREV_NORMAL_ROUGH=nr.copy(), PREV_DEPTH=prev_depth, PREV_MATERIAL=material.copy(), PREV_ILLUM=prev_illum,
               PREV_FAST=prev_fast, PREV_HIST_LEN=prev_hist.astype(np.float32), HIST_LEN=hist.astype(np.float32),
               ILLUM=illum, DEPTH=depth, NORMAL_ROUGH=nr, MATERIAL=material.astype(np.float32), ALBEDO=albedo,
               GEO_NORMAL_THIN=np.concatenate([nr[..., :3], np.zeros((h, w, 1), np.float32)], -1),
               MAT_PARAM=mat_param, MOTION=motion.astype(np.float32), RESERVOIRS=res, PING=ping, PONG=pong)
    for k, v in out.items():
        if k != "RESERVOIRS":
            assert v.dtype == np.float32 and np.isfinite(v).all(), k
    out.update(_sky=sky, _geo_in_sky=geo_in_sky, _sky_in_geo=sky_in_geo, _zero_normals=zero_n, _patches=patches,
               _disoccluded=dis, _dense_tile=dense_tile, _outliers=outliers, _lonely=lonely, _pair=pair,
               _motion_rows=dict(edge=row_edge, out=row_out), _subpixel=sub, _camera=cam.astype(np.float32),
               _history_values=hv)
    return out


def write_planes(dst, planes, ids=None):
    """Write every plane of make() to a vxpt.Renderer (ids None: by name) or an oracle.Oracle (ids = vxpt.BUF)."""
    for name in PLANES:
        dst.write(name if ids is None else ids[name], planes[name])
