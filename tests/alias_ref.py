"""Independent restatement of the parallel alias construction, a float32 FIFO Vose, and the
reconstruction error both tables are judged by.

The construction is written from its specification, in Python integers and numpy float64 / float32
scalars, with plain sequential loops:

  sum   = float32 of a float64 sum of the weights, taken in the documented tree order: chunks of 1024
          consecutive weights (padded with +0.0); within a chunk lane t of 256 adds weights 4t .. 4t+3 in
          order from 0.0, then the 256 lane values fold by halving (h = 128 .. 1: v[t] += v[t + h]);
          lane t of 256 then adds chunk sums t, t + 256, .. in order from 0.0 and the lanes fold the same way
  p[i]  = w[i] / sum, s[i] = p[i] * n, both binary32
  F[i]  = s[i] in fixed point, 40 fraction bits, round to nearest even (exact rational arithmetic);
          an s that is not finite, or above 2^22, counts as exactly 1
  lights s < 1 and heavies s >= 1 in index order; D_k = sum of (1 - s) over the first k lights,
  E_j = sum of (s - 1) over heavies 0 .. j
  light k: q = s, alias = heavy of the smallest j with E_j >= D_k; none: q = 1, alias = -1
  heavy j: K = smallest index with D_K > E_j; if K and heavy j + 1 exist: q = 1 + E_j - D_K as
           binary32, alias = heavy j + 1 (-1 when that q rounds to 1: the alias would never be
           taken, and -1 then marks exactly the bins with q == 1); else q = 1, alias = -1
"""
from fractions import Fraction

import numpy as np

FRAC = 40
ONE = 1 << FRAC


def _fold(v):
    v = list(v)
    h = len(v) // 2
    while h >= 1:
        for t in range(h):
            v[t] = np.float64(v[t] + v[t + h])
        h //= 2
    return v[0]


def tree_sum(w):
    w = np.asarray(w, np.float32)
    n = len(w)
    chunks = (n + 1023) // 1024
    pad = np.zeros(chunks * 1024, np.float64)
    pad[:n] = w.astype(np.float64)
    part = []
    for c in range(chunks):
        lanes = []
        for t in range(256):
            a = np.float64(0.0)
            for k in range(4):
                a = np.float64(a + pad[c * 1024 + 4 * t + k])
            lanes.append(a)
        part.append(_fold(lanes))
    lanes = []
    for t in range(256):
        a = np.float64(0.0)
        for c in range(t, chunks, 256):
            a = np.float64(a + part[c])
        lanes.append(a)
    return _fold(lanes)


def _fixed(s):
    s = float(s)
    if not np.isfinite(s) or abs(s) > 4194304.0:
        return ONE
    return round(Fraction(s) * ONE)  # Python's round of a Fraction: nearest, ties to even


def build(w):
    """-> q (float32), p (float32), alias (int32), sum (float32)"""
    w = np.asarray(w, np.float32)
    n = len(w)
    with np.errstate(all="ignore"):
        fsum = np.float32(tree_sum(w))
        p = (w / fsum).astype(np.float32)
        s = (p * np.float32(n)).astype(np.float32)
    lights, heavies, D, E = [], [], [0], []
    for i in range(n):
        if s[i] < np.float32(1.0):
            lights.append(i)
            D.append(D[-1] + (ONE - _fixed(s[i])))
        else:
            heavies.append(i)
            E.append((E[-1] if E else 0) + (_fixed(s[i]) - ONE))
    q = np.zeros(n, np.float32)
    alias = np.zeros(n, np.int32)
    for k, i in enumerate(lights):
        j = _first(E, lambda e: e >= D[k])
        if j is None:
            q[i], alias[i] = 1.0, -1
        else:
            q[i], alias[i] = s[i], heavies[j]
    for j, i in enumerate(heavies):
        K = _first(D, lambda d: d > E[j])
        if K is not None and j + 1 < len(heavies):
            q[i] = np.float32(np.float64(ONE + E[j] - D[K]) / np.float64(ONE))  # < 2^53: exact, then one rounding
            alias[i] = heavies[j + 1] if q[i] < np.float32(1.0) else -1  # never taken when q rounds to 1
        else:
            q[i], alias[i] = 1.0, -1
    return q, p, alias, fsum


def _first(a, pred):
    """smallest index of the monotone list a at which pred turns true, None if never"""
    lo, hi = 0, len(a)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(a[mid]):
            hi = mid
        else:
            lo = mid + 1
    return lo if lo < len(a) else None


def vose(w):
    """float32 FIFO Vose (two queues, index order): q, p, alias, sum"""
    w = np.asarray(w, np.float32)
    n = len(w)
    with np.errstate(all="ignore"):
        fsum = np.float32(np.sum(w.astype(np.float64)))
        p = (w / fsum).astype(np.float32)
        sc = (p * np.float32(n)).astype(np.float32)
    alias = np.full(n, -1, np.int32)
    small = [i for i in range(n) if sc[i] < 1.0]
    large = [i for i in range(n) if not sc[i] < 1.0]
    si = li = 0
    one = np.float32(1.0)
    while si < len(small) and li < len(large):
        s_, l_ = small[si], large[li]
        si += 1
        li += 1
        alias[s_] = l_
        sc[l_] = np.float32(sc[l_] - np.float32(one - sc[s_]))
        (small if sc[l_] < 1.0 else large).append(l_)
    for i in small[si:]:
        sc[i] = 1.0
    for i in large[li:]:
        sc[i] = 1.0
    return sc, p, alias, fsum


def recon_error(p, q, alias):
    """max_i |(q_i + sum_{alias_j = i} (1 - q_j)) / n - p_i| * n, in float64"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    alias = np.asarray(alias)
    n = len(p)
    mass = q.copy()
    has = alias >= 0
    np.add.at(mass, alias[has], 1.0 - q[has])
    return float(np.max(np.abs(mass / n - p) * n))


def check_valid(q, alias, p=None):
    """q in [0, 1]; alias in range, or -1 exactly where q == 1; no alias points to a light"""
    q, alias = np.asarray(q), np.asarray(alias)
    n = len(q)
    assert np.all((q >= 0.0) & (q <= 1.0)), "q outside [0, 1]"
    assert np.all((alias >= -1) & (alias < n)), "alias out of range"
    assert np.array_equal(alias == -1, q == 1.0), "alias is -1 exactly where q == 1"
    if p is not None:  # a light is a bin with s = p * n < 1
        s = (np.asarray(p, np.float32) * np.float32(n)).astype(np.float32)
        tgt = alias[alias >= 0]
        assert not np.any(s[tgt] < 1.0), "an alias points to a light"
