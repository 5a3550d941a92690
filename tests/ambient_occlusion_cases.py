"""Inputs shared by tests/test_ambient_occlusion_model.py (no GPU) and tests/test_ambient_occlusion_gpu.py (include/ovr_hip.h ovr_hip_set_ambient_occlusion,
DESIGN.md section 20): a ramp along x - a planar level set, in front of which nothing occludes -, a radial-distance volume whose level sets are spheres seen
from their centre - a cavity, where everything occludes -, their cameras and a seeded ray set.  Everything is cached and read-only."""
import numpy as np

F = np.float32
INF = float("inf")
RAMP_DIMS, CAVITY_N = (24, 20, 16), 32
SIZE = (24, 18)                       # frames of the model tests; the GPU tests take up to 48 x 36
FOVY = 60.0
KS = (1, 5, 16)
CAVITY_RADIUS, OUTER_RADIUS = 10.0, 12.0          # voxels; the volume holds r / CAVITY_N
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def ramp(dtype=np.float32):
    """value = (x + 0.5) / nx along x, constant in y and z: the level set 0.5 is the plane x = nx / 2"""
    key = ("ramp", np.dtype(dtype).name)
    if key not in _cache:
        nx, ny, nz = RAMP_DIMS
        v = np.broadcast_to(((np.arange(nx) + 0.5) / nx)[None, None, :], (nz, ny, nx))
        _cache[key] = _frozen(_quantize(v, dtype))
    return _cache[key]


def cavity(dtype=np.float32):
    """value = r / n, r the distance in voxels from the volume's centre (voxel centres at i + 0.5): the level set r0 / n is a sphere of radius r0"""
    key = ("cavity", np.dtype(dtype).name)
    if key not in _cache:
        n = CAVITY_N
        z, y, x = np.meshgrid(*(np.arange(n) + 0.5,) * 3, indexing="ij")
        r = np.sqrt((x - n / 2.0) ** 2 + (y - n / 2.0) ** 2 + (z - n / 2.0) ** 2)
        _cache[key] = _frozen(_quantize(np.clip(r / n, 0.0, 1.0), dtype))
    return _cache[key]


def _quantize(v, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.ascontiguousarray(np.rint(v * 255.0).astype(np.uint8))
    if dtype == np.uint16:
        return np.ascontiguousarray(np.rint(v * 65535.0).astype(np.uint16))
    return np.ascontiguousarray(v.astype(np.float32))


def level(radius, dtype=np.float32):
    """the isovalue of the sphere of that radius, in the units of the type's samples"""
    s = 65535.0 if np.dtype(dtype) == np.uint16 else 1.0
    return F(radius / CAVITY_N * s)


# (from, at, up)
RAMP_CAMERA = ((-8.0, 12.0, 9.5), (12.0, 10.0, 8.0), (0.0, 1.0, 0.0))           # looks at the plane from its low side
CAVITY_CAMERA = ((16.0, 16.0, 16.0), (26.0, 21.0, 19.0), (0.0, 1.0, 0.0))         # at the cavity's centre


def cavity_rays(n=96, seed=21):
    """seeded rays from points within two voxels of the cavity's centre, in every direction"""
    key = ("rays", n, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        org = 16.0 + rng.uniform(-2.0, 2.0, size=(n, 3))
        _cache[key] = (_frozen(org.astype(F)), _frozen(d.astype(F)))
    return _cache[key]
