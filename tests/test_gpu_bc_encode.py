"""The block encoders on the device (csrc/bcn_encode.hip) against their host twin: the same bytes
from Renderer.bc_encode and vxpt.bc_encode at quality 1 on every shape that takes another path
through the kernels, and the search load of a texture set (load_textures_bc(encoder="search")):
its uncached levels are the host's quality-1 blocks, its cached levels the files' bytes, the
expanding load samples bit-equal to the block sampler, and a plain load afterwards gives the fast
encoder's blocks again.
"""
import os

import numpy as np
import pytest

import vxpt
from golden.make_golden import C1_CAMERA
from test_bc_encode_search import bc4_six_value_blocks, mode5_blocks, two_line_blocks
from test_textures import _synthetic, make_data_dir, mip_chain, rgba0
from test_textures_bc import CACHED, FMT_OF_CH, SHORT, _cache_blocks, _probe_points, _renderer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plain():
    r = vxpt.Renderer(16, 16)
    yield r
    r.close()


def _shapes():
    rng = np.random.default_rng(17)
    yield "4x4", rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)        # one block: a lone wave in its workgroup
    yield "8x20", rng.integers(0, 256, (20, 8, 4), dtype=np.uint8)      # 10 blocks: a tail of 2
    yield "16x16", rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    for smooth in (True, False):
        yield "64x64 " + ("smooth" if smooth else "noisy"), np.ascontiguousarray(
            rgba0(_synthetic(np.random.default_rng(40 + smooth), 64, 4, smooth=smooth)))
    yield "two lines, left / right", two_line_blocks(True)
    yield "two lines, top / bottom", two_line_blocks(False)
    yield "mode 5", mode5_blocks()
    yield "six-value", bc4_six_value_blocks()


@pytest.mark.parametrize("kind", ["bc7 opaque", "bc7 alpha", "bc5", "bc4"])
def test_device_encode_equals_host(plain, kind):
    fmt = {"bc7 opaque": vxpt.BC7, "bc7 alpha": vxpt.BC7, "bc5": vxpt.BC5, "bc4": vxpt.BC4}[kind]
    with pytest.raises(vxpt.VxptError):
        plain.bc_encode(fmt, np.zeros((6, 8, 4), np.uint8))  # a height of 6
    with pytest.raises(vxpt.VxptError):
        plain.bc_encode(fmt, np.zeros((8, 8, 4), np.uint8), quality=2)
    for name, img in _shapes():
        img = img.copy()
        if kind == "bc7 opaque":
            img[..., 3] = 255
        for q in (1, 0):
            got = plain.bc_encode(fmt, img, quality=q)
            np.testing.assert_array_equal(got, vxpt.bc_encode(fmt, img, quality=q), err_msg="%s %s quality %d" % (kind, name, q))
    assert plain.bc_encode_ms() > 0.0


@pytest.fixture(scope="module")
def search_set(tmp_path_factory):
    golden = np.load(os.path.join(HERE, "golden", "bcn_blocks.npz"))
    root = str(tmp_path_factory.mktemp("texdata_bc_search"))
    images = make_data_dir(root)
    cache = os.path.join(root, "cache")
    os.makedirs(cache)
    files = {}
    for lod in range(6):
        blk = _cache_blocks(golden, ((128 >> lod) // 4) ** 2, lod)
        files[lod] = blk.reshape(-1)
        blk.tofile(vxpt.bc_cache_path(cache, CACHED, lod))
    np.zeros(64 * 64 // 16 * 16 - 1, np.uint8).tofile(vxpt.bc_cache_path(cache, SHORT, 0))
    cam = (C1_CAMERA[0], C1_CAMERA[1], C1_CAMERA[2])
    rb, rx = _renderer(root, cam), _renderer(root, cam)
    nb = rb.load_textures_bc(cache_dir=cache, encoder="search")
    nx = rx.load_textures_bc(cache_dir=cache, expand=True, encoder="search")
    expected = {}  # (path, level) -> host blocks at quality 1 (or the file's bytes), computed once
    for pth in sorted(images):
        img = images[pth]
        fmt = FMT_OF_CH[1 if img.ndim == 2 else img.shape[2]]
        for l, lv in enumerate(mip_chain(img)):
            expected[pth, l] = files[l] if pth == CACHED else vxpt.bc_encode(fmt, lv, quality=1)
    yield dict(bc=rb, ex=rx, images=images, files=files, loaded=(nb, nx), cache=cache, root=root, expected=expected)
    rb.close()
    rx.close()


def _check_blocks(r, images, expect):
    paths = sorted(images)
    table, total = r.texture_table_bc()
    blocks = r.read("TEX_BLOCKS")
    assert len(table) == len(paths) and blocks.size == total
    for i, pth in enumerate(paths):
        fmt, size, max_lod, offs = table[i]
        for l in range(max_lod + 1):
            exp = expect(pth, l, fmt)
            np.testing.assert_array_equal(blocks[offs[l]:offs[l] + exp.size], exp, err_msg="%s level %d" % (pth, l))


def test_search_load_blocks(search_set):
    r, images = search_set["bc"], search_set["images"]
    assert search_set["loaded"] == ((len(images), 6), (len(images), 6))  # the short file counts for nothing
    _check_blocks(r, images, lambda pth, l, fmt: search_set["expected"][pth, l])
    assert r.bc_encode_ms() > 0.0
    # nothing is written unasked
    assert sorted(os.listdir(search_set["cache"])) == sorted(
        os.path.basename(vxpt.bc_cache_path(search_set["cache"], p, l)) for p, l in [(CACHED, l) for l in range(6)] + [(SHORT, 0)])


def test_search_load_expanded_probes_bit_equal(search_set):
    rb, rx = search_set["bc"], search_set["ex"]
    table, total = rb.texture_table_bc()
    blocks = rb.read("TEX_BLOCKS")
    ttab, _ = rx.texture_table()
    texels = rx.read("TEXELS")
    for i, (fmt, size, max_lod, offs) in enumerate(table):
        for l in range(max_lod + 1):
            s = size >> l
            n = (s // 4) ** 2 * vxpt.bc_bytes_per_block(fmt)
            img = vxpt.bc_decode(fmt, blocks[offs[l]:offs[l] + n], s // 4, s // 4)
            got = texels[ttab[i][2][l]:ttab[i][2][l] + s * s].reshape(img.shape)
            np.testing.assert_array_equal(got, img, err_msg="texture %d level %d" % (i, l))
        pts = _probe_points(size, max_lod, 300 + i)
        a, b = rb.probe_texture(i, pts), rx.probe_texture(i, pts)
        assert np.isfinite(a).all()
        bad = a.view(np.uint32) != b.view(np.uint32)
        assert not bad.any(), (i, int(bad.any(axis=1).sum()), pts[bad.any(axis=1)][:4])


def test_search_set_renders_and_plain_load_restores_fast_blocks(search_set, tmp_path):
    r, images, files = search_set["bc"], search_set["images"], search_set["files"]
    r.trace(0)
    assert np.isfinite(r.read("ILLUM")).all()
    assert r.read("ALBEDO")[..., :3].std() > 0.05  # the textures really modulate the albedo
    # a search load that writes its cache: the files hold the quality-1 blocks, and a later load, with
    # or without the bit, takes them verbatim
    wc = str(tmp_path / "written")
    os.makedirs(wc)
    assert r.load_textures_bc(cache_dir=wc, write_cache=True, encoder="search") == (len(images), 0)
    q1 = {}  # every level of every texture at quality 1 (the fixture's, plus the texture it took from files)

    def host_q1(pth, l, fmt):
        if (pth, l) not in q1:
            q1[pth, l] = vxpt.bc_encode(fmt, mip_chain(images[pth])[l], quality=1) if pth == CACHED else search_set["expected"][pth, l]
        return q1[pth, l]

    _check_blocks(r, images, host_q1)
    for i, pth in enumerate(sorted(images)):
        fmt = r.texture_table_bc()[0][i][0]
        for l in range(len(mip_chain(images[pth]))):
            np.testing.assert_array_equal(np.fromfile(vxpt.bc_cache_path(wc, pth, l), np.uint8), host_q1(pth, l, fmt))
    n_levels = sum(len(mip_chain(images[p])) for p in images)
    assert r.load_textures_bc(cache_dir=wc) == (len(images), n_levels)
    _check_blocks(r, images, host_q1)
    assert r.load_textures_bc(cache_dir=wc, encoder="search") == (len(images), n_levels)
    _check_blocks(r, images, host_q1)
    # a plain load: the fast encoder's blocks again (and the cache files of the fixture)
    assert r.load_textures_bc(cache_dir=search_set["cache"]) == (len(images), 6)
    _check_blocks(r, images, lambda pth, l, fmt: files[l] if pth == CACHED else vxpt.bc_encode(fmt, mip_chain(images[pth])[l]))
    r.load_textures_bc(cache_dir=search_set["cache"], encoder="search")  # as the fixture left it

