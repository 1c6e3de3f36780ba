"""The world's DDA tables by their definitions, in numpy: an independent statement for the device
build's bodies (csrc/world_build.hpp).  The empty cubes and boxes are found by looking at the bricks
of each candidate box -- no prefix counts, no recurrence.

Layouts (csrc/vx_internal.hpp WorldDev): chunk-major ids x + 32 * (z + 32 * y) per 32^3 chunk, chunks
x-major, then z, then y; bricks of 4^3 cells indexed by 16^3 macro cell, then brick.
"""
import numpy as np


def grid(ids, chunks):
    """chunk-major ids -> [y][z][x] array of the whole world"""
    cx, cy, cz = chunks
    g = np.asarray(ids, np.uint8).reshape(cy, cz, cx, 32, 32, 32)  # chunk y, z, x, cell y, z, x
    return g.transpose(0, 3, 1, 4, 2, 5).reshape(cy * 32, cz * 32, cx * 32)


def brick_lin(chunks, bx, by, bz):
    mx, mz = chunks[0] * 2, chunks[2] * 2
    m = (bx >> 2) + mx * ((bz >> 2) + mz * (by >> 2))
    return m * 64 + (bx & 3) + 4 * ((bz & 3) + 4 * (by & 3))


def structures(ids, chunks):
    """-> dict BRICK_IDS, CELL_MASKS, MACRO_MASKS, SKY_TOP and occ ([by][bz][bx] bool)"""
    cx, cy, cz = chunks
    BX, BY, BZ = cx * 8, cy * 8, cz * 8
    g = grid(ids, chunks)
    cells = g.reshape(BY, 4, BZ, 4, BX, 4).transpose(0, 2, 4, 1, 3, 5).reshape(BY, BZ, BX, 64)  # cell y, z, x
    by, bz, bx = np.meshgrid(np.arange(BY), np.arange(BZ), np.arange(BX), indexing="ij")
    lin = brick_lin(chunks, bx, by, bz)
    nb = BX * BY * BZ
    brick_ids = np.zeros((nb, 64), np.uint8)
    brick_ids[lin.ravel()] = cells.reshape(nb, 64)
    cube = (cells >= 1) & (cells <= 12)
    masks = (cube.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    cell_masks = np.zeros(nb, np.uint64)
    cell_masks[lin.ravel()] = masks.ravel()
    occ = masks != 0
    macro = np.zeros(nb // 64, np.uint64)
    np.bitwise_or.at(macro, (lin // 64)[occ], np.uint64(1) << (lin % 64).astype(np.uint64)[occ])
    # column tops: 1 + the highest cube cell row of each brick column
    gc = (g >= 1) & (g <= 12)
    rows = np.where(gc, np.arange(1, cy * 32 + 1)[:, None, None], 0).max(0)  # [z][x] cells
    col = rows.reshape(BZ, 4, BX, 4).max((1, 3))
    sky = np.zeros((4, BZ, BX), np.uint16)
    for q in range(4):
        for z in range(BZ):
            for x in range(BX):
                xs = slice(x, None) if q & 1 else slice(0, x + 1)
                zs = slice(z, None) if q & 2 else slice(0, z + 1)
                sky[q, z, x] = col[zs, xs].max()
    return dict(BRICK_IDS=brick_ids.ravel(), CELL_MASKS=cell_masks, MACRO_MASKS=macro, SKY_TOP=sky, occ=occ)


def _flip(occ, octant):
    """the occupancy seen from the octant: every axis of the result points along the ray"""
    o = occ
    if not octant & 2:
        o = o[::-1]
    if not octant & 4:
        o = o[:, ::-1]
    if not octant & 1:
        o = o[:, :, ::-1]
    return o


def cube_and_box(occ, octant, bx, by, bz, cap, cap_up):
    """One (brick, octant): the cube edge (the largest s <= 255 whose s-cube, clamped to the grid, holds
    no occupied brick; 0 = occupied) and the box grown from it along x, z, y (csrc/box_tables.hpp)."""
    BY, BZ, BX = occ.shape
    o = _flip(occ, octant)
    x = bx if octant & 1 else BX - 1 - bx
    y = by if octant & 2 else BY - 1 - by
    z = bz if octant & 4 else BZ - 1 - bz
    if o[y, z, x]:
        return 0, 0

    def empty(ex, ey, ez):
        return not o[y:y + ey, z:z + ez, x:x + ex].any()

    s = 1
    while s < 255 and empty(s + 1, s + 1, s + 1):
        s += 1
        if x + s >= BX and y + s >= BY and z + s >= BZ:  # nothing more to meet
            s = 255
    e = [s, s, s]  # x, y, z
    pos, n = (x, y, z), (BX, BY, BZ)
    for a in (0, 2, 1):
        lim = min(255, max(s, cap_up if (a == 1 and octant & 2) else cap))
        while e[a] < lim and pos[a] + e[a] < n[a]:
            t = list(e)
            t[a] += 1
            if not empty(*t):
                break
            e = t
    return s, e[0] | (e[1] << 8) | (e[2] << 16)


def pairs(chunks, limit=4096, seed=17):
    """every (bx, by, bz, octant), or `limit` of them drawn with a fixed seed"""
    BX, BY, BZ = chunks[0] * 8, chunks[1] * 8, chunks[2] * 8
    n = BX * BY * BZ * 8
    k = np.arange(n) if n <= limit else np.random.default_rng(seed).choice(n, limit, replace=False)
    return [(int(i % BX), int(i // BX % BY), int(i // (BX * BY) % BZ), int(i // (BX * BY * BZ))) for i in k]
