"""Inputs shared by tests/test_isosurface_model.py (no GPU) and tests/test_isosurface_gpu.py: projection_cases' volumes, rays, cameras and tables, a centred ball,
the isovalues per volume and a float64 restatement of the trilinear field (include/ovr_hip.h ovr_hip_set_isosurfaces).  Everything is cached and read-only."""
import numpy as np

import projection_cases as PC

F = np.float32
DIMS, SIZE, RATES, DTYPES, CAMERAS, FOVY = PC.DIMS, PC.SIZE, PC.RATES, PC.DTYPES, PC.CAMERAS, PC.FOVY
KINDS = ("smooth", "slab", "plateau", "twin", "ball")
# isovalues as fractions of the type's full scale (scaled()); plateau: a level k / 255 exactly (101 / 255 is a plateau of the volume) and one between two levels
ISOVALUES = {
    "smooth": (0.31, 0.52, 0.74),
    "slab": (0.5, 0.8),
    "plateau": (101.0 / 255.0, 0.6),
    "twin": (0.4, 0.11),
    "ball": (0.4, 0.23, 0.61),
}
NESTED = {"smooth": (0.3, 0.45, 0.6, 0.75), "ball": (0.2, 0.35, 0.5, 0.65)}
BEHIND = ((20.0, 16.5, 78.0), (20.0, 16.5, 9.0), (0.0, 1.0, 0.0))   # a camera behind the volume: its rays cross the slab volume's dim cells (z >= 15) before the slab
BALL_RADIUS = 0.6   # R of value = clamp(1 - r / R), as a fraction of the smallest dimension
_cache = {}


def volume(kind, dtype=np.float32, dims=DIMS[0]):
    """projection_cases' volumes, and `ball`: value = clamp(1 - r / R) around the volume's centre (voxel centres at i + 0.5), R = BALL_RADIUS * min(dims)"""
    if kind != "ball":
        return PC.volume(kind, dtype, dims)
    key = (kind, np.dtype(dtype).name, tuple(dims))
    if key not in _cache:
        nx, ny, nz = dims
        z, y, x = np.meshgrid(np.arange(nz) + 0.5, np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing="ij")
        r = np.sqrt((x - nx / 2.0) ** 2 + (y - ny / 2.0) ** 2 + (z - nz / 2.0) ** 2)
        v = PC._quantize(np.clip(1.0 - r / (BALL_RADIUS * min(dims)), 0.0, 1.0), dtype)
        _cache[key] = PC._frozen(np.ascontiguousarray(v))
    return _cache[key]


def nonfinite_volume(dims=DIMS[0]):
    """the smooth f32 volume with 30 NaN, 30 +Inf and 30 -Inf voxels near its level sets"""
    key = ("nonfinite", tuple(dims))
    if key not in _cache:
        v = PC.volume("smooth", np.float32, dims).copy()
        nx, ny, nz = dims
        rng = np.random.default_rng([16, nx, ny, nz])
        near = np.argwhere((v > 0.4) & (v < 0.8))      # around the level sets the tests draw: the walks, the refinement and the gradient taps meet them
        pick = near[rng.choice(len(near), 90, replace=False)]
        for k, value in enumerate((np.nan, np.inf, -np.inf)):
            for z, y, x in pick[30 * k:30 * k + 30]:
                v[z, y, x] = value
        _cache[key] = PC._frozen(v)
    return _cache[key]


def scaled(values, dtype):
    """isovalues given as fractions of full scale, in the units of the type's samples: u16 raw, u8 and f32 as they are; float32"""
    s = 65535.0 if np.dtype(dtype) == np.uint16 else 1.0
    return np.sort((np.asarray(values, np.float64) * s).astype(F))


def sample64(volume, po):
    """the trilinear field of projection.sample in float64 (clamp-to-edge texels, cell-centred), at float64 object positions po (n, 3)"""
    v = np.asarray(volume)
    v = v.astype(np.float64) / 255.0 if v.dtype == np.uint8 else v.astype(np.float64)
    nz, ny, nx = v.shape
    x = np.clip(np.asarray(po, np.float64), 0.0, 1.0) * np.array([nx, ny, nz], np.float64) - 0.5
    i0 = np.floor(x).astype(np.int64)
    f = x - i0
    c = [(np.clip(i0[:, k], 0, n - 1), np.clip(i0[:, k] + 1, 0, n - 1)) for k, n in enumerate((nx, ny, nz))]

    def lerp(a, b, t):
        return a + t * (b - a)

    (x0, x1), (y0, y1), (z0, z1) = c
    c00, c10 = lerp(v[z0, y0, x0], v[z0, y0, x1], f[:, 0]), lerp(v[z0, y1, x0], v[z0, y1, x1], f[:, 0])
    c01, c11 = lerp(v[z1, y0, x0], v[z1, y0, x1], f[:, 0]), lerp(v[z1, y1, x0], v[z1, y1, x1], f[:, 0])
    return lerp(lerp(c00, c10, f[:, 1]), lerp(c01, c11, f[:, 1]), f[:, 2])


def root64(volume, org, direction, ta, tb, iso):
    """the float64 crossing of the level iso on [ta, tb] of each ray, found the way the model brackets it (two rounds of four points, the first sub-interval whose
    ends lie on different sides) and then bisected to 1e-9 of the interval; NaN where the ends do not lie on different sides"""
    v = np.asarray(volume)
    nz, ny, nx = v.shape
    inv = 1.0 / np.array([nx, ny, nz], np.float64)
    o, d = np.asarray(org, np.float64), np.asarray(direction, np.float64)
    iso = np.asarray(iso, np.float64)

    def field(t):
        return sample64(v, (o + t[:, None] * d) * inv)

    a, b = np.asarray(ta, np.float64).copy(), np.asarray(tb, np.float64).copy()
    width = b - a
    fa, fb = field(a), field(b)
    ok = (iso <= fa) != (iso <= fb)
    for _ in range(2):
        p = [a] + [a + c * (b - a) for c in (0.2, 0.4, 0.6, 0.8)] + [b]
        q = [fa] + [field(x) for x in p[1:5]] + [fb]
        na, nb, nfa, nfb, done = a.copy(), b.copy(), fa.copy(), fb.copy(), np.zeros(a.shape, bool)
        for j in range(5):
            take = ~done & ((iso <= q[j]) != (iso <= q[j + 1]))
            na, nfa, nb, nfb = np.where(take, p[j], na), np.where(take, q[j], nfa), np.where(take, p[j + 1], nb), np.where(take, q[j + 1], nfb)
            done |= take
        a, b, fa, fb = na, nb, nfa, nfb
    for _ in range(40):
        m = 0.5 * (a + b)
        fm = field(m)
        left = (iso <= fa) != (iso <= fm)
        b, fb = np.where(left, m, b), np.where(left, fm, fb)
        a, fa = np.where(left, a, m), np.where(left, fa, fm)
        if ((b - a) <= 1e-9 * width).all():
            break
    return np.where(ok, 0.5 * (a + b), np.nan)
