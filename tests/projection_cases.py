"""Inputs shared by tests/test_projection_model.py (no GPU) and tests/test_projection_gpu.py: the volumes, the ray set, the transfer functions and the cameras of
the projection tests (include/ovr_hip.h ovr_hip_set_projection).  Everything is generated from seeds and cached; the arrays are read-only."""
import numpy as np

F = np.float32
DIMS = ((40, 33, 18), (24, 20, 17))   # (nx, ny, nz): 3 x 3 x 2 macrocells, no axis a multiple of a brick or a cell; and a single-cell-deep one
SIZE = (40, 28)                       # ragged 8 x 8 blocks
RATES = (1.0, 2.5)
DTYPES = (np.float32, np.uint16, np.uint8)
CAMERAS = {  # eye, at, up; fovy 40.  World = voxel units of the 40 x 33 x 18 volume
    "oblique": ((-31.5, 44.25, -39.0), (20.0, 16.5, 9.0), (0.0, 1.0, 0.0)),
    "axis": ((20.0, 16.5, -60.0), (20.0, 16.5, 9.0), (0.0, 1.0, 0.0)),
}
FOVY = 40.0
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _quantize(v, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.rint(np.clip(v, 0, 1) * 255.0).astype(np.uint8)
    if dtype == np.uint16:
        return np.rint(np.clip(v, 0, 1) * 65535.0).astype(np.uint16)
    return v.astype(F)


def volume(kind, dtype=np.float32, dims=DIMS[0]):
    """(nz, ny, nx) arrays.  random: white noise in [0, 1) (f32: shifted to [-0.5, 0.5), so that magnitudes and widths differ); smooth: a blob plus noise (the
    threshold identity's); plateau: every 16^3 block constant at one of a few levels k / 255, the block maxima equal to neighbouring blocks' values; slab: a bright
    slab at low z in front of a dim rest; twin: the same maximum in two cells along z"""
    key = (kind, np.dtype(dtype).name, tuple(dims))
    if key in _cache:
        return _cache[key]
    nx, ny, nz = dims
    rng = np.random.default_rng([{"random": 11, "smooth": 12, "plateau": 13, "slab": 14, "twin": 15}[kind], nx, ny, nz])   # (the same field for every voxel type)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if kind == "random":
        v = rng.random((nz, ny, nx))
        if np.dtype(dtype) == np.float32:
            v = v - 0.5
    elif kind == "smooth":
        r2 = ((x - 0.55 * nx) / nx) ** 2 + ((y - 0.45 * ny) / ny) ** 2 + ((z - 0.5 * nz) / nz) ** 2
        v = np.clip(1.0 - 2.0 * np.sqrt(r2), 0.0, 1.0) * 0.9 + 0.05 * rng.random((nz, ny, nx))
    elif kind == "plateau":
        levels = np.array([37, 37, 101, 101, 200, 254, 255]) / 255.0
        blocks = levels[rng.integers(0, len(levels), ((nz + 15) // 16 + 1, (ny + 15) // 16 + 1, (nx + 15) // 16 + 1))]
        # the plateaus are offset by 5 voxels from the macrocell grid: every cell sees its neighbours' levels
        v = blocks[(z + 5) // 16, (y + 5) // 16, (x + 5) // 16]
    elif kind == "slab":
        v = 0.1 + 0.1 * rng.random((nz, ny, nx))
        v[1:4] = 0.9 + 0.05 * rng.random((3, ny, nx))
    elif kind == "twin":
        v = 0.2 * rng.random((nz, ny, nx))
        v[3, :, :] = 0.75
        v[nz - 2, :, :] = 0.75   # the other macrocell along z holds the same maximum
    else:
        raise ValueError(kind)
    _cache[key] = _frozen(np.ascontiguousarray(_quantize(v, dtype)))
    return _cache[key]


def ray_set(dims, seed=5):
    """world rays (org, dir) for a volume of dims voxels at spacing 1, origin 0: random rays through the box, axis-parallel rays with zero direction components,
    corner grazers with fewer than 4 steps at rate 1, rays from inside, misses.  Returns (org (n, 3), dir (n, 3), kind (n,) names)"""
    key = ("rays", tuple(dims), seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    n = np.array(dims, np.float64)
    org, d, kind = [], [], []

    def add(o, v, k, normalise=True):
        v = np.asarray(v, np.float64)
        if normalise:
            v = v / np.linalg.norm(v)
        org.append(np.asarray(o, np.float64)); d.append(v); kind.append(k)

    for _ in range(48):   # through the box
        a, b = rng.random(3) * n, rng.random(3) * n
        v = (b - a) / np.linalg.norm(b - a)
        add(a - v * (10.0 + 60.0 * rng.random()), v, "through")
    for ax in range(3):   # axis-parallel: two zero components, then one
        for _ in range(4):
            p = rng.random(3) * n
            v = np.zeros(3); v[ax] = rng.choice([-1.0, 1.0])
            add(p - v * (n[ax] + 7.25), v, "axis")
            w = rng.standard_normal(3); w[ax] = 0.0
            add(rng.random(3) * n - w / np.linalg.norm(w) * 80.0, w, "axis")
    for c in range(8):    # corner grazers: a chord of 0.6 ... 3 voxels across an edge at the corner
        corner = np.array([(c >> k) & 1 for k in range(3)]) * n
        inward = np.where(corner > 0, -1.0, 1.0)
        e = 0.4 + 1.6 * rng.random()
        a = corner + inward * np.array([e, 0.0, 0.7]); b = corner + inward * np.array([0.0, e, 1.1])
        v = (b - a) / np.linalg.norm(b - a)
        add(a - v * 25.0, v, "grazer")
    for _ in range(12):   # from inside
        add(rng.random(3) * n, rng.standard_normal(3), "inside")
    for _ in range(8):    # misses
        p = rng.random(3) * n
        add(p + np.array([0.0, 0.0, n[2] + 20.0]), [rng.standard_normal(), rng.standard_normal(), 1.0 + rng.random()], "miss")
    out = (_frozen(np.array(org, F)), _frozen(np.array(d, F)), np.array(kind))
    _cache[key] = out
    return out


def transfer_function(ovr, kind, dtype, n=16):
    """(colors flat 3 n, alphas flat (pos, alpha) 2 n, value_range): `sparse` is monotone non-decreasing (0 below 40 %, a ramp to 0.6 at 80 %); `zero`: the
    all-zero alpha table, under which the march never terminates early"""
    colors, alphas, vr = ovr.synth.make_tfn("sparse", n, dtype)
    if np.dtype(dtype) == np.float32 and kind != "unit":
        vr = (-0.5, 1.0)   # covers the shifted random volume
    alphas = np.array(alphas, F).copy()
    if kind == "zero":
        alphas[1::2] = 0.0
    return colors, alphas, vr


def tables(colors, alphas):
    """the tables as committed: colours (n, 3), alphas (n,) - the positions of the app-side format are not read"""
    return np.asarray(colors, F).reshape(-1, 3), np.asarray(alphas, F).reshape(-1, 2)[:, 1].copy()
