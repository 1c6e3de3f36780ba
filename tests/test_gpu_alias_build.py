"""The alias kernels (vxpt_alias_build) against the host twin (vxpt_alias_build_host), bit for bit: the
CPU test's sizes and weights, the two real table sizes (1024 x 512 and 32 x 32), and sizes around the
kernels' boundaries -- 1024 bins per workgroup, and 256 workgroup sums (262144 bins) per round of the
one-workgroup scan of the sums."""
import numpy as np
import pytest

import vxpt
from test_alias_build import KINDS, SIZES, weights

pytestmark = pytest.mark.gpu

EDGES = (1023, 1025, 2048, 262143, 262144, 262145)


@pytest.fixture(scope="module")
def renderer():
    r = vxpt.Renderer(64, 36)
    yield r
    r.close()


def _same(dev, host, tag):
    for name, a, b in zip(("q", "p", "alias", "sum"), dev, host):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


@pytest.mark.parametrize("kind", KINDS)
def test_kernels_equal_the_twin(renderer, kind):
    for n in SIZES:
        w = weights(kind, n)
        _same(renderer.alias_build(w), vxpt.alias_build_host(w), (kind, n))


@pytest.mark.parametrize("n", EDGES + (32 * 32, 1024 * 512))
def test_kernels_equal_the_twin_at_the_boundaries(renderer, n):
    w = weights("lognormal", n)
    _same(renderer.alias_build(w), vxpt.alias_build_host(w), n)


def test_half_zero_sky_sized_table_and_repeat(renderer):
    w = weights("half_zeros", 1024 * 512)
    first = renderer.alias_build(w)
    _same(first, vxpt.alias_build_host(w), "half_zeros")
    _same(renderer.alias_build(weights("one_hot", 4097)), vxpt.alias_build_host(weights("one_hot", 4097)), "between")
    _same(renderer.alias_build(w), first, "repeat")  # the scratch buffers are reused: nothing stale is read
