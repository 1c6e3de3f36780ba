"""Block-compressed textures (TextureManager.cu:189-330): BC7 / BC5 / BC4 mip chains decoded in
the sampler, the reference's cache files, the deterministic encoder.

CPU: the host decode (the body the sampler runs) against tests/golden/bcn_blocks.npz -- random
blocks with the RGBA a DDS reader decodes them to (make_bcn_golden.py) -- the reserved BC7 mode,
the encoder's determinism and error bound, the cache-file naming and size rule.
GPU: the loader's block buffer against the host encoder and the cache files; the block sampler
bit-equal to the RGBA8 sampler on the host-decoded texels (vxpt_probe_texture); frames bit-equal
between the two and within the textured bars of the oracle given the decoded chains.
"""
import os

import numpy as np
import pytest

import oracle
import vxpt
from golden.make_golden import C1_CAMERA
from test_gpu_parity import E_MAX_TEXTURED, _compare_radiance, _inject_sky, DN_FLOATS, DN_INTS
from test_textures import KINDS, TEX, _synthetic, make_data_dir, mip_chain, rgba0

HERE = os.path.dirname(os.path.abspath(__file__))
FMT_OF_CH = {1: vxpt.BC4, 2: vxpt.BC5, 3: vxpt.BC7, 4: vxpt.BC7}
# the G-buffer bar of test_textures.test_textured_frames_match_oracle (inline there)
G_RTOL = G_ATOL = 2e-4
G_BAD = 1e-3
CACHED = "textures/cliff_a.png"   # the texture whose levels come from cache files (BC7, 128 px, 6 levels)
SHORT = "textures/sand_a.png"     # its level-0 cache file is one byte short: ignored


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "bcn_blocks.npz"))


def _per_block(img, nbx, nby):
    return img.reshape(nby, 4, nbx, 4, 4).swapaxes(1, 2).reshape(nby * nbx, 4, 4, 4)


# ------------------------------------------------------------------ CPU
def test_bc_decode_matches_fixture(golden):
    for m in range(8):
        got = _per_block(vxpt.bc_decode(vxpt.BC7, golden["bc7_blocks"][m], 64, 1), 64, 1)
        np.testing.assert_array_equal(got, golden["bc7_rgba"][m], err_msg="BC7 mode %d" % m)
    b5 = _per_block(vxpt.bc_decode(vxpt.BC5, golden["bc5_blocks"], 16, 16), 16, 16)
    np.testing.assert_array_equal(b5[..., :2], golden["bc5_rg"])
    assert (b5[..., 2] == 0).all() and (b5[..., 3] == 255).all()
    b4 = _per_block(vxpt.bc_decode(vxpt.BC4, golden["bc4_blocks"], 16, 16), 16, 16)
    np.testing.assert_array_equal(b4[..., 0], golden["bc4_r"])
    assert (b4[..., 1] == 0).all() and (b4[..., 2] == 0).all() and (b4[..., 3] == 255).all()
    # the fixture holds the cases the issue names
    e0, e1 = golden["bc4_blocks"][:, 0].astype(int), golden["bc4_blocks"][:, 1].astype(int)
    idx = np.array([[(int.from_bytes(bytes(b[2:]), "little") >> (3 * t)) & 7 for t in range(16)]
                    for b in golden["bc4_blocks"]])
    assert (e0 > e1).any() and (e0 == e1).any()
    assert ((e0 < e1)[:, None] & (idx == 6)).any() and ((e0 < e1)[:, None] & (idx == 7)).any()
    assert (golden["bc7_blocks"][..., 0] != 0).all()
    for m in range(8):
        assert ((golden["bc7_blocks"][m, :, 0] & ((2 << m) - 1)) == (1 << m)).all()


def test_bc7_reserved_mode_decodes_to_zero():
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    blocks[:, 0] = 0
    assert (vxpt.bc_decode(vxpt.BC7, blocks, 4, 4) == 0).all()


def _block_stats(img, dec, nch):
    """per block: largest absolute error, largest deviation from the block's own mean colour"""
    h, w = img.shape[:2]
    a = _per_block(img, w // 4, h // 4)[..., :nch].astype(np.float64)
    d = _per_block(dec, w // 4, h // 4)[..., :nch].astype(np.float64)
    err = np.abs(a - d).max(axis=(1, 2, 3))
    dev = np.abs(a - a.mean(axis=(1, 2), keepdims=True)).max(axis=(1, 2, 3))
    return err, dev


def test_bc_encoder():
    rng = np.random.default_rng(3)
    const = np.zeros((8, 8, 4), np.uint8)
    const[...] = (13, 200, 77, 255)
    for fmt, nch in ((vxpt.BC7, 4), (vxpt.BC5, 2), (vxpt.BC4, 1)):
        noise = rng.integers(0, 256, (32, 32, 4), dtype=np.uint8)
        np.testing.assert_array_equal(vxpt.bc_encode(fmt, noise), vxpt.bc_encode(fmt, noise.copy()))
        d = vxpt.bc_decode(fmt, vxpt.bc_encode(fmt, const), 2, 2)
        err = np.abs(d[..., :nch].astype(int) - const[..., :nch]).max()
        # mode 6: an endpoint's four channels share one p-bit (the low bit of all four)
        assert err <= (1 if fmt == vxpt.BC7 else 0), (fmt, err)
    # the synthetic textures of test_textures.py: no block worse than its own mean colour would be
    for ch in (1, 2, 3, 4):
        for smooth in (True, False):
            for n in (16, 64):
                img = rgba0(_synthetic(np.random.default_rng(11 + n + ch), n, ch, smooth=smooth))
                fmt, nch = FMT_OF_CH[ch], {1: 1, 2: 2, 3: 4, 4: 4}[ch]
                dec = vxpt.bc_decode(fmt, vxpt.bc_encode(fmt, img), n // 4, n // 4)
                err, dev = _block_stats(img, dec, nch)
                rmse = np.sqrt(((dec[..., :nch].astype(np.float64) - img[..., :nch]) ** 2).mean())
                print("bc encode %d px %d ch %s: rmse %.3f, max %d" % (n, ch, "smooth" if smooth else "noisy", rmse,
                                                                        err.max()))
                assert (err <= dev + 1).all(), (n, ch, smooth, np.argmax(err - dev), (err - dev).max())


def test_bc_cache_files(tmp_path):
    cache = str(tmp_path / "cache")
    os.makedirs(cache)
    # <name>: what follows the path's first '/', up to ".png" (TextureManager.cu:168-173)
    assert vxpt.bc_cache_path(cache, "textures/sand_a.png", 3) == os.path.join(cache, "sand_a_lod_3.bin")
    assert vxpt.bc_cache_path(cache, "textures/sub/x.png", 0) == os.path.join(cache, "sub", "x_lod_0.bin")
    assert vxpt.bc_cache_path(cache, "plain.png", 1) == os.path.join(cache, "plain_lod_1.bin")
    rng = np.random.default_rng(9)
    img = rgba0(_synthetic(rng, 16, 3, smooth=False))
    for fmt in (vxpt.BC7, vxpt.BC5, vxpt.BC4):
        tex = "textures/t%d.png" % fmt
        enc = vxpt.bc_encode(fmt, img)
        got, hit = vxpt.bc_level(fmt, img, tex, 0, cache_dir=cache)
        assert not hit and (got == enc).all()
        assert not os.path.exists(vxpt.bc_cache_path(cache, tex, 0))  # nothing is written unasked
        # a file of exactly size^2 / 16 blocks is taken verbatim; pitch size / 4 x bytes per block
        blob = rng.integers(1, 256, enc.size, dtype=np.uint8)
        assert enc.size == 16 * vxpt.bc_bytes_per_block(fmt)
        blob.tofile(vxpt.bc_cache_path(cache, tex, 0))
        got, hit = vxpt.bc_level(fmt, img, tex, 0, cache_dir=cache)
        assert hit and (got == blob).all()
        # any other size is ignored: one byte short, one byte long
        for n in (enc.size - 1, enc.size + 1):
            np.resize(blob, n).tofile(vxpt.bc_cache_path(cache, tex, 0))
            got, hit = vxpt.bc_level(fmt, img, tex, 0, cache_dir=cache)
            assert not hit and (got == enc).all()
        # VXPT_TEX_WRITE_CACHE writes the encoded level, which the next call then reads
        got, hit = vxpt.bc_level(fmt, img, tex, 1, cache_dir=cache, write_cache=True)
        assert not hit and (np.fromfile(vxpt.bc_cache_path(cache, tex, 1), np.uint8) == enc).all()
        assert vxpt.bc_level(fmt, img, tex, 1, cache_dir=cache)[1]


# ------------------------------------------------------------------ GPU
def _cache_blocks(golden, n_blocks, lod):
    """n BC7 blocks from the fixture, every mode present (level 0 of the 128 px texture: all 512, twice)"""
    flat = golden["bc7_blocks"].transpose(1, 0, 2).reshape(512, 16)  # mode varies fastest
    return np.resize(np.roll(flat, -8 * lod, axis=0), (n_blocks, 16))


def _renderer(root, cam):
    r = vxpt.Renderer(128, 96, data_dir=root)
    r.load_settings()
    r.generate_terrain((2, 1, 2), height_scale=32.0)
    r.set_camera(*cam[:2], fov=cam[2], prev=cam)
    r.set_sky(0.25, 45.0, 0.0, 1.0)
    return r


@pytest.fixture(scope="module")
def bc_pair(tmp_path_factory, golden):
    root = str(tmp_path_factory.mktemp("texdata_bc"))
    images = make_data_dir(root)
    cache = os.path.join(root, "cache")
    os.makedirs(cache)
    files = {}
    for lod in range(6):
        s = 128 >> lod
        blk = _cache_blocks(golden, (s // 4) ** 2, lod)
        files[lod] = blk.reshape(-1)
        blk.tofile(vxpt.bc_cache_path(cache, CACHED, lod))
    np.zeros(64 * 64 // 16 * 16 - 1, np.uint8).tofile(vxpt.bc_cache_path(cache, SHORT, 0))
    cam = (C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2])
    rb, rx = _renderer(root, cam), _renderer(root, cam)
    nb = rb.load_textures_bc(cache_dir=cache)
    nx = rx.load_textures_bc(cache_dir=cache, expand=True)
    yield dict(bc=rb, ex=rx, images=images, files=files, loaded=(nb, nx), cam=cam)
    rb.close()
    rx.close()


def _decoded_chains(r):
    """every texture's levels decoded from the context's TEX_BLOCKS by the fixture-checked host decode"""
    table, total = r.texture_table_bc()
    blocks = r.read("TEX_BLOCKS")
    assert blocks.size == total
    out = []
    for fmt, size, max_lod, offs in table:
        lv = []
        for l in range(max_lod + 1):
            s = size >> l
            n = (s // 4) ** 2 * vxpt.bc_bytes_per_block(fmt)
            lv.append(vxpt.bc_decode(fmt, blocks[offs[l]:offs[l] + n], s // 4, s // 4))
        out.append(lv)
    return out


@pytest.mark.gpu
def test_bc_loader_blocks(bc_pair):
    r, images, files = bc_pair["bc"], bc_pair["images"], bc_pair["files"]
    paths = sorted(images)
    assert bc_pair["loaded"] == ((len(paths), 6), (len(paths), 6))  # the short file counts for nothing
    table, total = r.texture_table_bc()
    assert len(table) == len(paths) and total % 16 == 0
    assert [(t[1], t[2]) for t in table] == [(t[0], t[1]) for t in r.texture_table()[0]]
    blocks = r.read("TEX_BLOCKS")
    for i, pth in enumerate(paths):
        fmt, size, max_lod, offs = table[i]
        img = images[pth]
        assert fmt == FMT_OF_CH[1 if img.ndim == 2 else img.shape[2]], pth
        chain = mip_chain(img)
        assert size == chain[0].shape[0] and max_lod == len(chain) - 1
        for l, lv in enumerate(chain):
            if fmt != vxpt.BC4:
                assert offs[l] % 16 == 0, (pth, l, offs[l])
            assert offs[l] % 8 == 0
            exp = files[l] if pth == CACHED else vxpt.bc_encode(fmt, lv)
            got = blocks[offs[l]:offs[l] + exp.size]
            np.testing.assert_array_equal(got, exp, err_msg="%s level %d" % (pth, l))
    # the block buffer is a quarter of the RGBA8 texels or less (BC4: an eighth), up to the chains' padding
    assert total <= r.texture_table()[1] + 16 * len(paths)


def _probe_points(size, max_lod, seed):
    """4096 (u, v, lod): uniform in [-2, 3) over every lod range; texel centres, texel borders and
    block borders of every level at that level's lod and beside it"""
    rng = np.random.default_rng(seed)
    n = 2048
    uni = np.stack([rng.uniform(-2, 3, n), rng.uniform(-2, 3, n), rng.uniform(-1.5, max_lod + 1.5, n)], -1)
    uni[:256, 2] = rng.integers(0, max_lod + 1, 256)     # integer lods
    uni[256:384, 2] = -0.75                              # below 0
    uni[384:512, 2] = max_lod + 0.5                      # above maxLod
    grid = []
    per = (4096 - n) // (max_lod + 1)
    for l in range(max_lod + 1):
        s = size >> l
        i, j = rng.integers(-s, 2 * s, per), rng.integers(-s, 2 * s, per)
        kind = np.arange(per) % 4
        off = np.where(kind == 0, 0.5, 0.0)                        # centre / border
        i = np.where(kind == 2, (i // 4) * 4, i)                   # block border
        j = np.where(kind >= 2, (j // 4) * 4, j)
        lod = l + np.choose(np.arange(per) % 3, [0.0, 0.25, -0.5])
        grid.append(np.stack([(i + off) / s, (j + off) / s, lod], -1))
    pts = np.concatenate([uni] + grid)
    pts = np.concatenate([pts, uni[:4096 - len(pts)] * [1, 1, 0] + [0.37, 0.11, 0]])
    assert pts.shape == (4096, 3)
    return pts.astype(np.float32)


@pytest.mark.gpu
def test_bc_sampler_bit_equal_to_expanded(bc_pair):
    rb, rx = bc_pair["bc"], bc_pair["ex"]
    chains = _decoded_chains(rb)
    table, _ = rx.texture_table()
    texels = rx.read("TEXELS")
    paths = sorted(bc_pair["images"])
    assert paths.index(CACHED) >= 0
    for i, lv in enumerate(chains):
        size, max_lod, offs = table[i]
        for l, img in enumerate(lv):
            got = texels[offs[l]:offs[l] + img.shape[0] * img.shape[1]].reshape(img.shape)
            np.testing.assert_array_equal(got, img, err_msg="%s level %d" % (paths[i], l))
        pts = _probe_points(size, max_lod, 100 + i)
        a, b = rb.probe_texture(i, pts), rx.probe_texture(i, pts)
        assert np.isfinite(a).all()
        bad = a.view(np.uint32) != b.view(np.uint32)
        assert not bad.any(), (paths[i], int(bad.any(axis=1).sum()), pts[bad.any(axis=1)][:4], a[bad][:4], b[bad][:4])
        # and the sampler really reads this texture: the level-0 texel centres give the texels
        s = size
        yy, xx = np.mgrid[0:4, 0:8]
        c = np.stack([(xx.ravel() + 0.5) / s, (yy.ravel() + 0.5) / s, np.zeros(32)], -1).astype(np.float32)
        want = lv[0][yy.ravel(), xx.ravel()].astype(np.float32) / np.float32(255.0)
        np.testing.assert_allclose(rb.probe_texture(i, c), want, rtol=0, atol=1e-6)


@pytest.mark.gpu
def test_bc_frames(bc_pair):
    rb, rx, cam = bc_pair["bc"], bc_pair["ex"], bc_pair["cam"]
    paths = sorted(bc_pair["images"])
    o = oracle.Oracle(rb.W, rb.H)
    o.terrain((2, 1, 2))
    o.set_camera(*cam[:2], fov=cam[2])
    o.set_camera(*cam[:2], fov=cam[2], which=1)
    o.set_denoise_params(DN_FLOATS, DN_INTS)
    o.set_textures(_decoded_chains(rb))
    for b, (_, kinds) in TEX.items():
        ids = [paths.index("textures/" + kinds[k][0]) if k in kinds else -1 for k in KINDS]
        o.set_material_textures(b, *ids, uv_scale=2.5, world_grid=True)
    _inject_sky(rb, o)
    p = vxpt.DenoiseParams(*DN_FLOATS, *DN_INTS)
    def both_equal(f):
        for name in ("ALBEDO", "NORMAL_ROUGH", "MAT_PARAM", "ILLUM", "OUTPUT"):
            a, b = rb.read(name), rx.read(name)
            assert (a.view(np.uint32) == b.view(np.uint32)).all(), (f, name, np.abs(a - b).max())

    # the flow of test_textures.test_textured_frames_match_oracle, on the block context
    rb.trace(0)
    rx.trace(0)
    o.trace(0)
    for name in ("DEPTH", "NORMAL_ROUGH", "ALBEDO", "MAT_PARAM", "GEO_NORMAL_THIN"):
        g, c = rb.read(name), o.read(vxpt.BUF[name])
        bad = ~np.isclose(g, c, rtol=G_RTOL, atol=G_ATOL)
        assert bad.mean() < G_BAD, (name, bad.mean(), np.argwhere(bad)[:5])
    assert rb.read("ALBEDO")[..., :3].std() > 0.05  # the textures really modulate the albedo
    _compare_radiance(rb.read("ILLUM"), o.read(0), "bc frame0", E_MAX_TEXTURED)
    rb.denoise(0, 1, p)
    rx.denoise(0, 1, p)
    o.post_trace()
    o.denoise(0, 1)
    both_equal(0)
    for f in range(1, 3):
        for r in (rb, rx):
            r.trace(f)
            r.denoise(f, f + 1, p)
        o.trace(f)
        o.post_trace()
        o.denoise(f, f + 1)
        _compare_radiance(rb.read("ILLUM"), o.read(0), "bc frame%d" % f, E_MAX_TEXTURED)
        _compare_radiance(rb.read("OUTPUT"), o.read(21), "bc output %d" % f, E_MAX_TEXTURED)
        both_equal(f)


@pytest.mark.gpu
def test_bc_enable_textures_toggle(bc_pair):
    r = bc_pair["bc"]
    r.enable_textures(False)
    r.trace(3)
    assert np.allclose(r.read("ALBEDO")[..., :3][r.read("DEPTH") < 1e20], 1.0)
    r.enable_textures(True)
    r.trace(4)
    assert r.read("ALBEDO")[..., :3].std() > 0.05
