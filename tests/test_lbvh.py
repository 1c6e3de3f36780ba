"""vxpt.lbvh_host, the host twin of the device TLAS builder (csrc/lbvh.hpp), against the numpy
restatement tests/lbvh_ref.py.  No GPU."""
import numpy as np
import pytest

import lbvh_ref
import vxpt

SIZES = (0, 1, 2, 3, 63, 64, 65, 1000)
LAYOUTS = ("random32", "random1024", "line", "two_per_cell", "corners")


def _instances(layout, n, seed):
    """n distinct (x, y, z, object) rows of the layout (fewer where the layout has fewer)."""
    rng = np.random.default_rng(seed)
    if layout in ("random32", "random1024"):
        side = 32 if layout == "random32" else 1024
        rows = set()
        while len(rows) < n:
            rows.add(tuple(int(v) for v in rng.integers(0, side, 3)) + (int(rng.integers(12, 29)),))
        rows = sorted(rows)
        rng.shuffle(rows)
    elif layout == "line":  # every cell of one axis line (at most 1024 of them)
        rows = [(5, int(x), 7, 13) for x in rng.permutation(1024)[:min(n, 1024)]]
    elif layout == "two_per_cell":  # keys that differ only in the low 5 bits
        cells = [tuple(int(v) for v in c) for c in rng.integers(0, 1024, (n // 2 + 1, 3))]
        rows = [c + (o,) for c in dict.fromkeys(cells) for o in (14, 15)][:n]
    else:  # every axis at 0 or 1023: 8 cells, 17 objects each
        rows = [(x, y, z, o) for x in (0, 1023) for y in (0, 1023) for z in (0, 1023) for o in range(12, 29)]
        rows = [rows[i] for i in rng.permutation(len(rows))[:min(n, len(rows))]]
    rows = np.array(rows, np.int64).reshape(-1, 4)
    cell = rows[:, :3].astype(np.float32)
    boxes = np.concatenate([cell - rng.random((len(rows), 3), np.float32) * np.float32(0.1),
                            cell + np.float32(1) + rng.random((len(rows), 3), np.float32) * np.float32(0.1)], 1)
    keys = np.array([vxpt.lbvh_key(*r) for r in rows], np.uint64)
    return rows, boxes.astype(np.float32), keys


def test_key_is_morton_then_object():
    assert vxpt.lbvh_key(0, 0, 0, 0) == 0
    assert vxpt.lbvh_key(1, 0, 0, 0) == 1 << 5 and vxpt.lbvh_key(0, 1, 0, 0) == 2 << 5
    assert vxpt.lbvh_key(0, 0, 1, 3) == (4 << 5) | 3
    assert vxpt.lbvh_key(1023, 1023, 1023, 31) == (1 << 35) - 1
    rng = np.random.default_rng(1)
    for x, y, z, o in rng.integers(0, (1024, 1024, 1024, 32), (50, 4)):
        m = sum(((int(x) >> b) & 1) << (3 * b) | ((int(y) >> b) & 1) << (3 * b + 1) | ((int(z) >> b) & 1) << (3 * b + 2)
                for b in range(10))
        assert vxpt.lbvh_key(x, y, z, o) == (m << 5) | int(o)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_lbvh_host_matches_restatement(layout, n):
    rows, boxes, keys = _instances(layout, n, seed=n * 7 + len(layout))
    n = len(rows)
    assert len(set(int(k) for k in keys)) == n
    nodes, order = vxpt.lbvh_host(boxes, keys)
    assert len(nodes) == max(2 * n - 1, 0)
    if n == 0:
        return
    # order is the key order
    assert sorted(order.tolist()) == list(range(n))
    assert (np.diff(keys[order].astype(np.int64)) > 0).all()
    # every instance in exactly one leaf, one instance per leaf
    leaves = nodes[nodes["count"] != 0]
    assert (leaves["count"] == 1).all() and sorted(leaves["left"].tolist()) == list(range(n))
    # node 0 is the root; the children of inner node i at 1 + 2i and 2 + 2i
    inner = nodes[nodes["count"] == 0]
    assert len(inner) == n - 1
    assert sorted(inner["left"].tolist()) == [1 + 2 * i for i in range(n - 1)]
    if n > 1:
        assert nodes[0]["count"] == 0 and nodes[0]["left"] == 1
    # bit-equal to the restatement: topology and every widened union
    ref, ref_order, depth = lbvh_ref.build(boxes, keys)
    np.testing.assert_array_equal(order, ref_order)
    assert nodes.tobytes() == ref.tobytes()
    assert depth <= 35
    # every parent encloses its children; the walk from the root reaches every leaf within 35 levels
    stack, seen = [(0, 0)], 0
    while stack:
        s, d = stack.pop()
        assert d <= 35
        if nodes[s]["count"]:
            seen += 1
            continue
        for c in (nodes[s]["left"], nodes[s]["left"] + 1):
            assert (nodes[c]["lo"] >= nodes[s]["lo"]).all() and (nodes[c]["hi"] <= nodes[s]["hi"]).all()
            stack.append((int(c), d + 1))
    assert seen == n


def test_lbvh_host_refuses_a_key_out_of_range():
    with pytest.raises(vxpt.VxptError):
        vxpt.lbvh_host(np.zeros((2, 6), np.float32), np.array([1, 1 << 35], np.uint64))


def test_large_worlds_keep_the_host_builder():
    """Device mode builds the TLAS on the device up to 1024 cells (32 chunks) on every axis."""
    assert vxpt.lbvh_world_fits((8, 8, 8)) and vxpt.lbvh_world_fits((32, 32, 32)) and vxpt.lbvh_world_fits((32, 1, 2))
    for ch in ((33, 1, 1), (1, 33, 1), (1, 1, 33), (64, 64, 64)):
        assert not vxpt.lbvh_world_fits(ch)
