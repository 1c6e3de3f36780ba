"""The index map of vxpt_set_render_size / vxpt_resize_host, stated independently in numpy: new pixel
(x, y) takes old pixel (sx, sy), the old pixel under the new pixel's centre.  In doubled coordinates
the centre of new pixel x is 2x + 1 of 2 * new_w, so the old pixel is floor((2x + 1) * old_w / (2 * new_w)),
evaluated exactly with integer floor division over index vectors (int64)."""
import numpy as np

# the issue's shapes: (old_w, old_h) -> (new_w, new_h)
SHAPES = (((96, 64), (64, 48)), ((64, 48), (96, 64)), ((50, 37), (33, 21)), ((33, 21), (50, 37)),
          ((7, 5), (7, 5)), ((1, 1), (5, 3)), ((5, 3), (1, 1)))
# pixel records: float planes, float4 planes, reservoirs (5 x 4 bytes)
PIXELS = {4: (np.float32, ()), 16: (np.float32, (4,)), 20: (np.uint32, (5,))}


def source_indices(old_n, new_n):
    centres = 2 * np.arange(new_n, dtype=np.int64) + 1
    return np.minimum(centres * old_n // (2 * new_n), old_n - 1)


def resize(arr, new_w, new_h):
    h, w = arr.shape[:2]
    return arr[source_indices(h, new_h)[:, None], source_indices(w, new_w)[None, :]]


def pattern(w, h, bpp, seed=0):
    """every value distinct per pixel and per component: a wrong pixel or a mixed record shows"""
    dtype, tail = PIXELS[bpp]
    n = int(np.prod(tail, dtype=np.int64)) if tail else 1
    v = np.arange(w * h * n, dtype=np.int64).reshape((h, w) + tail) * 7 + seed
    return v.astype(dtype)
