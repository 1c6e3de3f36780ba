"""An independent float32 restatement of the terrain generator (vxpt_terrain_host / the kernels of
csrc/terrain.hip), in numpy: MT19937 in plain Python, the permutation's shuffle, four octaves of the
improved Perlin noise, the column height with its one fused multiply-add, and the id rule.

Every step is a single correctly rounded float32 operation, as in the library (-ffp-contract=off);
the fused n * 1.4f - 0.7f is evaluated exactly (rationals) and rounded once.

It checks itself in two ways (check_mt19937, check_against_oracle): the generator's 10000th output for
the default seed 5489 and its first are the standard's, and the noise of seed 124 equals the oracle's.

CASES lists the shapes, seeds and origins the CPU and GPU terrain tests share.
"""
from fractions import Fraction

import numpy as np

BALLS, GLOBAL_Y = 1, 2
F = np.float32


class MT19937:
    """std::mt19937 (32-bit Mersenne Twister), plain Python."""

    def __init__(self, seed):
        self.s = [0] * 624
        self.s[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.s[i] = (1812433253 * (self.s[i - 1] ^ (self.s[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.i = 624

    def __call__(self):
        if self.i >= 624:
            s = self.s
            for k in range(624):
                y = (s[k] & 0x80000000) | (s[(k + 1) % 624] & 0x7FFFFFFF)
                s[k] = s[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.i = 0
        y = self.s[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def check_mt19937():
    g = MT19937(5489)
    first = g()
    assert first == 3499211612, first  # the standard's first output of the default seed
    for _ in range(9998):
        g()
    assert g() == 4123659995  # [rand.predef]: the 10000th invocation of a default mt19937


def permutation(seed):
    p = list(range(256))
    g = MT19937(seed)
    for i in range(1, 256):
        r = g() % (i + 1)
        p[i], p[r] = p[r], p[i]
    return np.array(p, np.int32)


def _fade(t):
    return t * t * t * (t * (t * F(6) - F(15)) + F(10))


def _lerp(a, b, t):
    return a + (b - a) * t


def _grad(h, x, y, z):
    h = h & 15
    u = np.where(h < 8, x, y)
    v = np.where(h < 4, y, np.where((h == 12) | (h == 14), x, z))
    return np.where((h & 1) == 0, u, -u) + np.where((h & 2) == 0, v, -v)


def noise(p, x, y, z):
    x, y, z = (np.asarray(a, F) for a in np.broadcast_arrays(x, y, z))
    X, Y, Z = np.floor(x), np.floor(y), np.floor(z)
    ix, iy, iz = (a.astype(np.int64) & 255 for a in (X, Y, Z))
    fx, fy, fz = x - X, y - Y, z - Z
    u, v, w = _fade(fx), _fade(fy), _fade(fz)
    one = F(1)
    A, B = (p[ix] + iy) & 255, (p[(ix + 1) & 255] + iy) & 255
    AA, AB = (p[A] + iz) & 255, (p[(A + 1) & 255] + iz) & 255
    BA, BB = (p[B] + iz) & 255, (p[(B + 1) & 255] + iz) & 255
    q0 = _lerp(_grad(p[AA], fx, fy, fz), _grad(p[BA], fx - one, fy, fz), u)
    q1 = _lerp(_grad(p[AB], fx, fy - one, fz), _grad(p[BB], fx - one, fy - one, fz), u)
    q2 = _lerp(_grad(p[(AA + 1) & 255], fx, fy, fz - one), _grad(p[(BA + 1) & 255], fx - one, fy, fz - one), u)
    q3 = _lerp(_grad(p[(AB + 1) & 255], fx, fy - one, fz - one), _grad(p[(BB + 1) & 255], fx - one, fy - one, fz - one), u)
    return _lerp(_lerp(q0, q1, v), _lerp(q2, q3, v), w)


def octave01(p, x, y, octaves=4):
    x, y = np.asarray(x, F).copy(), np.asarray(y, F).copy()
    r, a = np.zeros(np.broadcast(x, y).shape, F), F(1)
    for _ in range(octaves):
        r = r + noise(p, x, y, F(0.34567)) * a
        x, y, a = x * F(2), y * F(2), a * F(0.5)
    out = r * F(0.5) + F(0.5)
    out = np.where(F(1) <= r, F(1), out)
    return np.where(r <= F(-1), F(0), out).astype(F)


def _round_f32(q):
    """the float32 nearest the rational q (ties to even)"""
    c = F(float(q))
    best = None
    for cand in (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))):
        d = abs(Fraction(float(cand)) - q)
        even = (int(np.array(cand, F).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, cand)
    return best[1]


def _fmaf(n, a, b):
    a, b = Fraction(float(F(a))), Fraction(float(F(b)))
    return np.array([_round_f32(Fraction(float(v)) * a + b) for v in n.ravel()], F).reshape(n.shape)


def heights(chunks, height_scale, freq_den, origin, seed):
    """[z, x] column heights of the window"""
    p = permutation(seed)
    freq, width = F(1) / F(freq_den), F(height_scale)
    gx = (origin[0] + np.arange(chunks[0] * 32)).astype(F) * freq
    gz = (origin[2] + np.arange(chunks[2] * 32)).astype(F) * freq
    n = octave01(p, gx[None, :], gz[:, None], 4)
    h = _fmaf(n, 1.4, -0.7)
    h = np.maximum(F(0.1), (h + F(0.25)) * width)
    return np.minimum(h, width * F(0.9)).astype(F)


def generate(chunks=(2, 1, 2), height_scale=32.0, freq_den=None, flags=0, origin=(0, 0, 0), seed=124):
    """the chunk-major ids vxpt_terrain_host gives for the same arguments"""
    cx, cy, cz = chunks
    if freq_den is None:
        freq_den = 32.0 * cx
    width = F(height_scale)
    h = heights(chunks, height_scale, freq_den, origin, seed)[None, :, :]
    layer = np.repeat(np.arange(cy), 32) * 32 if flags & GLOBAL_Y else np.zeros(cy * 32, np.int64)
    local = np.tile(np.arange(32), cy)
    yy = (origin[1] + layer + local).astype(F)[:, None, None]
    d = h - yy
    low = h < width * (F(0.25) + F(0.05))
    mid = (h < width * (F(0.25) + F(0.6))) & (h > width * (F(0.25) + F(0.3)))
    ids = np.where(low, np.where(d < F(3.5), 1, 7),
                   np.where(mid, np.where(d < F(5.5), 3, 7), np.where(d < F(1.5), 2, np.where(d < F(5.5), 3, 7))))
    ids = np.where(yy < h, ids, 0).astype(np.uint8)
    if flags & BALLS:
        ball = [17, 21, 22, 23, 24, 25, 26, 27, 28, 29]
        for gx in range(30, 40):
            x, z = gx - origin[0], 43 - origin[2]
            if 0 <= x < cx * 32 and 0 <= z < cz * 32:
                ids[local == 7, z, x] = ball[gx - 30]
    # [y, z, x] -> chunks x-major, then z, then y; x + 32 * (z + 32 * y) in a chunk
    return np.ascontiguousarray(ids.reshape(cy, 32, cz, 32, cx, 32).transpose(0, 2, 4, 1, 3, 5)).reshape(-1)


def check_against_oracle(n=2000):
    import oracle
    p = permutation(124)
    rng = np.random.default_rng(1)
    x, y = (rng.uniform(-40.0, 40.0, n).astype(F) for _ in range(2))
    mine = octave01(p, x, y, 4)
    theirs = np.array([oracle.perlin(float(a), float(b), 4) for a, b in zip(x, y)], F)
    np.testing.assert_array_equal(mine.view(np.uint32), theirs.view(np.uint32))


def chunk(ids, chunks, c):
    """the 32768 ids of chunk c = (x, y, z) of a chunk-major world"""
    k = c[0] + chunks[0] * (c[2] + chunks[2] * c[1])
    return ids[k * 32768:(k + 1) * 32768]


# (chunks, height_scale, freq_den, flags): origin 0 and seed 124, the oracle's terrain
ORACLE_CASES = [((1, 1, 1), 32.0, None, 0), ((2, 1, 2), 32.0, None, 0), ((3, 2, 1), 32.0, None, 0),
                ((1, 1, 1), 32.0, None, GLOBAL_Y), ((2, 1, 2), 32.0, None, GLOBAL_Y), ((3, 2, 1), 48.0, None, GLOBAL_Y),
                ((2, 1, 2), 32.0, None, BALLS)]  # the ball row x 30..39 straddles the chunk boundary at 32
# (chunks, height_scale, freq_den, flags, origin, seed): other worlds and windows
SEED_CASES = [((2, 1, 2), 128.0, 64.0, GLOBAL_Y, origin, seed)
              for seed, origin in ((0, (-37, 0, 1000)), (1, (32, 0, 0)), (2 ** 32 - 1, (5, 64, -5)),
                                   (0, (5, 64, -5)), (1, (-37, 0, 1000)), (2 ** 32 - 1, (32, 0, 0)))]
SEED_CASES += [((1, 2, 1), 80.0, 48.0, GLOBAL_Y | BALLS, (20, 16, 30), 7),  # balls inside a shifted window
               ((2, 2, 1), 32.0, 64.0, BALLS, (25, 0, 40), 124)]           # chunk-local y: balls in both layers
CASES = [c + ((0, 0, 0), 124) for c in ORACLE_CASES] + SEED_CASES
