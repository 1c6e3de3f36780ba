"""The terrain generator with an origin and a seed, on the host (vxpt_terrain_host; no GPU):
against the oracle's terrain for origin 0 and seed 124, against the independent numpy restatement
(terrain_ref.py) for other seeds and origins, the consistency of overlapping windows, and the
argument checks."""
import ctypes

import numpy as np
import pytest

import oracle
import terrain_ref as T
import vxpt


def _host(case):
    chunks, hs, fd, flags, origin, seed = case
    return vxpt.terrain_host(chunks, hs, fd, flags, origin, seed)


def test_reference_checks_itself():
    T.check_mt19937()
    T.check_against_oracle()


@pytest.mark.parametrize("case", T.ORACLE_CASES, ids=str)
def test_origin_0_seed_124_equals_the_oracle(case):
    chunks, hs, fd, flags = case
    o = oracle.Oracle(8, 8)
    o.terrain(chunks, height_scale=hs, freq_den=fd, use_fma=True, keep_balls=bool(flags & T.BALLS),
              global_y=bool(flags & T.GLOBAL_Y))
    ids = _host(case + ((0, 0, 0), 124))
    np.testing.assert_array_equal(ids, o.voxels())
    assert 0 < np.count_nonzero(ids) < ids.size
    if flags & T.BALLS:  # the row straddles the chunk boundary at x = 32
        assert set(np.unique(ids)) >= {17, 21, 29}
        assert T.chunk(ids, chunks, (0, 0, 1)).max() >= 17 and T.chunk(ids, chunks, (1, 0, 1)).max() >= 17


@pytest.mark.parametrize("case", T.CASES, ids=str)
def test_equals_the_numpy_restatement(case):
    ids = _host(case)
    np.testing.assert_array_equal(ids, T.generate(*case))


def test_seeds_and_origins_give_other_worlds():
    base = T.SEED_CASES[0]
    worlds = [_host(base[:4] + (origin, seed)) for origin, seed in (((0, 0, 0), 124), ((0, 0, 0), 0), ((32, 0, 0), 124))]
    assert all(0 < np.count_nonzero(w) < w.size for w in worlds)
    assert not np.array_equal(worlds[0], worlds[1]) and not np.array_equal(worlds[0], worlds[2])


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("seed", [124, 0])
def test_a_shifted_window_is_a_chunk_of_the_larger_world(axis, seed):
    """one freq_den: a (1,1,1) world 32 cells along the axis is chunk 1 of the two-chunk world at origin 0"""
    big = [1, 1, 1]
    big[axis] = 2
    at = [0, 0, 0]
    at[axis] = 1
    flags = T.GLOBAL_Y if axis == 1 else 0
    whole = vxpt.terrain_host(tuple(big), 96.0, 64.0, flags, (0, 0, 0), seed)
    part = vxpt.terrain_host((1, 1, 1), 96.0, 64.0, flags, tuple(32 * v for v in at), seed)
    np.testing.assert_array_equal(part, T.chunk(whole, big, at))
    assert 0 < np.count_nonzero(part) < part.size
    assert not np.array_equal(part, T.chunk(whole, big, (0, 0, 0)))


LIM = 1 << 24
BAD = [
    dict(chunks=(0, 1, 1)), dict(chunks=(1, -1, 1)), dict(chunks=(1, 1, 0)),
    dict(freq_den=0.0),
    dict(origin=(0, 1, 0)), dict(origin=(0, -32, 0)),                # y without GLOBAL_Y
    dict(origin=(LIM, 0, 0)), dict(origin=(0, 0, -LIM)), dict(origin=(0, LIM, 0), flags=T.GLOBAL_Y),
    dict(origin=(LIM - 32, 0, 0)), dict(origin=(0, 0, LIM - 63), chunks=(1, 1, 2)),  # origin + extent reaches 2^24
    dict(origin=(0, LIM - 32, 0), flags=T.GLOBAL_Y),
    dict(origin=(-(LIM + 5), 0, 0)),
]


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_bad_descriptors_are_refused(bad):
    a = dict(chunks=(1, 1, 1), height_scale=32.0, freq_den=32.0, flags=0, origin=(0, 0, 0), seed=124)
    a.update(bad)
    lib = vxpt.load_library()
    d = vxpt.TerrainDesc((ctypes.c_int * 3)(*a["chunks"]), a["height_scale"], a["freq_den"], a["flags"],
                         (ctypes.c_int * 3)(*a["origin"]), a["seed"])
    ids = np.full(2 * 32768, 255, np.uint8)
    assert lib.vxpt_terrain_host(ctypes.byref(d), ids.ctypes.data) == -1  # VXPT_ERR_ARG
    assert (ids == 255).all()
    with pytest.raises(vxpt.VxptError):
        vxpt.terrain_host(**a)


def test_null_arguments_and_the_last_exact_window():
    lib = vxpt.load_library()
    ids = np.zeros(32768, np.uint8)
    d = vxpt.TerrainDesc((ctypes.c_int * 3)(1, 1, 1), 32.0, 32.0, 0, (ctypes.c_int * 3)(0, 0, 0), 124)
    assert lib.vxpt_terrain_host(None, ids.ctypes.data) == -1
    assert lib.vxpt_terrain_host(ctypes.byref(d), None) == -1
    # the last window whose coordinates all stay below 2^24, and the first above -2^24
    for origin in ((LIM - 33, 0, 0), (0, 0, -(LIM - 1))):
        case = ((1, 1, 1), 32.0, 32.0, 0, origin, 124)
        np.testing.assert_array_equal(_host(case), T.generate(*case))
