"""Inputs shared by tests/test_camera_model.py (no GPU) and tests/test_camera_gpu.py: the cross-section volume and its two cameras, an oblique and an axis
camera around a 24^3 ball, small transfer-function tables.  Everything is cached and read-only."""
import numpy as np

import isosurface_cases as IC

F = np.float32
_cache = {}

# ---- the cross-section case: v[z, y, x] = g[y, x], seen along -z at one pixel per voxel - every projection of the volume IS g
XDIMS = (32, 16, 8)
XCAM = ((16.0, 8.0, 20.0), (16.0, 8.0, 4.0), (0.0, 1.0, 0.0))
XFRAMES = (((32, 16), 16.0), ((64, 32), 32.0))   # (size, orthographic height): the volume fills the first frame, the second has a margin of 16 / 8 pixels
XRATES = (1.0, 0.7, 2.5)


def _frozen(a):
    a.setflags(write=False)
    return a


def cross_section():
    """g (16, 32): small integers, none of them 0, no two neighbours equal"""
    if "g" not in _cache:
        y, x = np.mgrid[0:XDIMS[1], 0:XDIMS[0]]
        _cache["g"] = _frozen(((x * 7 + y * 13) % 23 + 1).astype(np.int64))
    return _cache["g"]


def cross_section_volume(dtype=np.float32):
    key = ("xvol", np.dtype(dtype).name)
    if key not in _cache:
        g = cross_section().astype(dtype)
        _cache[key] = _frozen(np.ascontiguousarray(np.broadcast_to(g[None], (XDIMS[2], XDIMS[1], XDIMS[0]))))
    return _cache[key]


def inner(size):
    """the slices of the volume's silhouette in the second frame"""
    w, h = size
    return slice((h - XDIMS[1]) // 2, (h + XDIMS[1]) // 2), slice((w - XDIMS[0]) // 2, (w + XDIMS[0]) // 2)


# ---- the ball: a 24^3 volume under an oblique and an axis camera, frames with ragged 8 x 8 blocks
BDIMS = (24, 24, 24)
BSIZE = (44, 28)
OBLIQUE = ((47.0, 38.0, 52.0), (12.0, 12.0, 12.0), (0.0, 1.0, 0.0))
AXIS = ((12.0, 12.0, 60.0), (12.0, 12.0, 12.0), (0.0, 1.0, 0.0))
BHEIGHT = 36.0   # the ball's box (24 high, ~41.6 across its diagonal) with a margin: misses on every side of the 44 x 28 frame's width


def ball(dtype=np.float32):
    return IC.volume("ball", dtype, BDIMS)


def tables(n=64):
    """a colour table (n, 3) and an alpha table (n,) that rise with the value, and their (position, alpha) pairs as set_transfer_function takes them"""
    key = ("tf", n)
    if key not in _cache:
        x = np.linspace(0.0, 1.0, n).astype(F)
        colors = np.stack([x, (1 - x) * x * 4, 1 - x], 1).astype(F)
        alphas = (0.05 + 0.9 * x).astype(F)
        pairs = np.stack([x, alphas], 1).astype(F)
        _cache[key] = tuple(_frozen(a) for a in (colors, alphas, pairs))
    return _cache[key]
