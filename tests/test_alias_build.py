"""The parallel alias construction's host twin (vxpt_alias_build_host) against its float64 / integer
restatement (alias_ref.build), and its tables against float32 FIFO Vose on the same weights.

q is compared bit for bit, not within an ulp: the only float operation after the integer part is the
conversion of a 41-bit integer to binary32, which both sides do through a double (exact below 2^53) and
one round-to-nearest-even; nothing is left to differ.

Reconstruction bar: the twin's recon_error <= 2 x Vose's + n * 2^-40 (the fixed point's own
resolution summed over the bins), measured against Vose, never against the twin itself.
"""
import numpy as np
import pytest

import alias_ref
import oracle
import vxpt

SIZES = (1, 2, 3, 63, 64, 65, 257, 1000, 1024, 4097)
KINDS = ("uniform", "one_hot", "half_zeros", "lognormal", "one_huge", "all_equal_but_one")


def weights(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, n).astype(np.float32)
    if kind == "one_hot":
        w = np.zeros(n, np.float32)
        w[(7 * n) // 11] = 3.0
        return w
    if kind == "half_zeros":
        w = rng.uniform(0.1, 1.0, n).astype(np.float32)
        w[rng.permutation(n)[: n // 2]] = 0.0
        if not w.any():
            w[0] = 1.0
        return w
    if kind == "lognormal":
        return rng.lognormal(0.0, 2.0, n).astype(np.float32)
    if kind == "one_huge":
        w = rng.uniform(0.5, 1.0, n).astype(np.float32)
        w[n // 3] *= np.float32(1e5)
        return w
    if kind == "all_equal_but_one":
        w = np.full(n, 0.37, np.float32)
        w[n - 1] = 0.91
        return w
    raise ValueError(kind)


_cache = {}


def tables(kind, n):
    """(weights, twin, ref, vose), each computed once"""
    key = (kind, n)
    if key not in _cache:
        w = weights(kind, n)
        _cache[key] = (w, vxpt.alias_build_host(w), alias_ref.build(w), alias_ref.vose(w))
    return _cache[key]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def check_against_vose(w, table, vose):
    q, p, alias, _ = table
    n = len(w)
    alias_ref.check_valid(q, alias, p)
    err = alias_ref.recon_error(p, q, alias)
    verr = alias_ref.recon_error(vose[1], vose[0], vose[2])
    assert err <= 2.0 * verr + n * 2.0 ** -40, (err, verr)
    return err, verr


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_equals_reference(kind, n):
    w, twin, ref, _ = tables(kind, n)
    assert np.array_equal(twin[2], ref[2]), "alias"
    assert np.array_equal(bits(twin[1]), bits(ref[1])), "p"
    assert bits(twin[3]) == bits(ref[3]), "sum"
    assert np.array_equal(bits(twin[0]), bits(ref[0])), "q"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_valid_and_reconstructs(kind, n):
    w, twin, _, vose = tables(kind, n)
    err, verr = check_against_vose(w, twin, vose)
    print("recon %s n=%d: twin %.3e vose %.3e ratio %.3f" % (kind, n, err, verr, err / verr if verr else 0.0))


@pytest.mark.parametrize("kind,n", [("lognormal", 4097), ("half_zeros", 1000), ("one_hot", 65)])
def test_twin_repeats(kind, n):
    w, twin, _, _ = tables(kind, n)
    again = vxpt.alias_build_host(w)
    for a, b in zip(twin, again):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_oracle_sky_pdf():
    """the oracle's sky table probabilities (proportional to its sky pdf), every 128th texel"""
    o = oracle.Oracle(8, 8)
    o.set_sky()
    w = np.ascontiguousarray(o.sky()["p"].reshape(-1)[5::128], np.float32)
    assert len(w) == 4096 and w.sum() > 0
    twin, ref, vose = vxpt.alias_build_host(w), alias_ref.build(w), alias_ref.vose(w)
    for a, b in zip(twin, ref):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    check_against_vose(w, twin, vose)


def test_rejects_bad_sizes():
    with pytest.raises(vxpt.VxptError):
        vxpt.alias_build_host(np.zeros(0, np.float32))
