"""A plain numpy restatement of the linear BVH of csrc/lbvh.hpp, written for the tests.

Sort the primitives by key (ties, which the instance set never has, by index); a range of sorted
primitives splits where the highest bit in which its first and last key differ turns from 0 to 1;
recurse.  Node 0 is the root; the inner node that covers a range is numbered by the range's end when it
is a left child and by its start when it is a right child (the root is 0), and keeps its children at
1 + 2i and 2 + 2i.  A node's box is the float32 min / max union of its primitives' boxes, widened once
by 1e-4 (1 + |coordinate|) in float32.
"""
import numpy as np

NODE = np.dtype([("lo", "<f4", 3), ("left", "<i4"), ("hi", "<f4", 3), ("count", "<i4")])
INDEX_BITS = 29


def widen(lo, hi):
    e, one = np.float32(1e-4), np.float32(1.0)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return lo - e * (one + np.abs(lo)), hi + e * (one + np.abs(hi))


def build(boxes, keys):
    """-> (nodes [2n - 1] NODE, order [n], depth of the deepest leaf)."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    n = len(boxes)
    words = [(int(k) << INDEX_BITS) | i for i, k in enumerate(keys)]
    order = sorted(range(n), key=lambda i: words[i])
    w = [words[i] for i in order]
    nodes = np.zeros(max(2 * n - 1, 0), NODE)
    deepest = [0]

    def put(slot, first, last, left, count):
        b = boxes[order[first:last + 1]]
        nodes[slot]["lo"], nodes[slot]["hi"] = widen(b[:, :3].min(0), b[:, 3:].max(0))
        nodes[slot]["left"], nodes[slot]["count"] = left, count

    def rec(slot, first, last, index, depth):
        if first == last:
            put(slot, first, last, first, 1)
            deepest[0] = max(deepest[0], depth)
            return
        bit = (w[first] ^ w[last]).bit_length() - 1
        split = max(i for i in range(first, last) if not (w[i] >> bit) & 1)
        put(slot, first, last, 1 + 2 * index, 0)
        rec(1 + 2 * index, first, split, split, depth + 1)
        rec(2 + 2 * index, split + 1, last, split + 1, depth + 1)

    if n:
        rec(0, 0, n - 1, 0, 0)
    return nodes, np.array(order, np.int32), deepest[0]
