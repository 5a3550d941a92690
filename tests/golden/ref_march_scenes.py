"""The fixed scene list of tests/golden/ref_march.npz, shared by the generator (make_ref_march.py) and the tests that read the fixture.

Everything here is reproducible bit for bit on any machine: volumes come from integer arithmetic on a seeded integer lattice (numpy's
PCG64 stream is stable), tables and cameras from a handful of IEEE basic operations.  The fixture still stores every small input
(tables, camera, grid, pixel list) and a CRC of each volume, so a test notices if its regenerated input is not what the generator fed
the reference."""
import zlib

import numpy as np

DTYPES = {"u8": np.uint8, "i8": np.int8, "u16": np.uint16, "i16": np.int16, "u32": np.uint32, "i32": np.int32, "f32": np.float32, "f64": np.float64}
REF_VALUE_TYPE = {"u8": 100, "i8": 101, "u16": 200, "i16": 201, "u32": 300, "i32": 301, "f32": 400, "f64": 500}   # ovr/scene.h, pinned by ref_probe.json


def make_volume(seed, dims, dtype, const_region=False):
    """trilinear upsampling of a 5^3 lattice of random 16-bit integers, in exact integer arithmetic; shape (nz, ny, nx).  const_region: the
    lower half in z is one value - zero gradient there, so the marcher's normal is NaN and must be dropped by its clamp."""
    nx, ny, nz = dims
    lat = np.random.default_rng(seed).integers(0, 65536, size=(5, 5, 5), dtype=np.int64)
    def axis(n):
        u = (np.arange(n, dtype=np.int64) * (4 * 256)) // max(n - 1, 1)   # fixed point, 8 fractional bits, in [0, 4]
        c = np.minimum(u >> 8, 3)
        return c, u - (c << 8)
    (cx, fx), (cy, fy), (cz, fz) = axis(nx), axis(ny), axis(nz)
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.zeros((nz, ny, nx), dtype=np.int64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (fx[X] if dx else 256 - fx[X]) * (fy[Y] if dy else 256 - fy[Y]) * (fz[Z] if dz else 256 - fz[Z])
                v += w * lat[cz[Z] + dz, cy[Y] + dy, cx[X] + dx]
    v >>= 24   # 0 .. 65535
    if const_region:
        v[: nz // 2] = 40000
    dtype = np.dtype(DTYPES[dtype])
    if dtype == np.uint8:
        return (v >> 8).astype(np.uint8)
    if dtype == np.int8:
        return ((v >> 8) - 128).astype(np.int8)
    if dtype == np.uint16:
        return v.astype(np.uint16)
    if dtype == np.int16:
        return (v - 32768).astype(np.int16)
    if dtype == np.uint32:
        return (v * 65537).astype(np.uint32)
    if dtype == np.int32:
        return (v * 65537 - 2147483648).astype(np.int32)
    if dtype == np.float32:
        return (v / 65535.0).astype(np.float32)
    return v / 65535.0


def make_tables(n_colors, n_alphas, kind):
    """(colours flat rgb, alphas flat (position, alpha)) in the app-side format of set_transfer_function"""
    r = np.arange(n_colors, dtype=np.float64) / max(n_colors - 1, 1)
    colors = np.stack([r, 1.0 - np.abs(2.0 * r - 1.0), 1.0 - r], axis=1).astype(np.float32)
    p = np.arange(n_alphas, dtype=np.float64) / max(n_alphas - 1, 1)
    if kind == "ramp":
        a = 0.9 * p
    elif kind == "sparse":   # nothing below 40 %, up to 0.6 at 80 %
        a = np.minimum(np.maximum((p - 0.4) / 0.4, 0.0), 1.0) * 0.6
    elif kind == "bumps":
        a = np.zeros_like(p)
        for c, w, h in ((0.35, 0.06, 0.3), (0.6, 0.08, 0.5), (0.85, 0.1, 0.8)):
            a = np.maximum(a, h * np.minimum(np.maximum(1.0 - np.abs(p - c) / w, 0.0), 1.0))
    elif kind == "thin":   # low opacity everywhere: long marches, no early termination
        a = 0.02 + 0.05 * p
    else:
        raise ValueError(kind)
    alphas = np.stack([p, a], axis=1).astype(np.float32)
    return colors.ravel(), alphas.ravel()


def make_camera(kind, dims, spacing, origin):
    ext = np.array(spacing, np.float64) * np.array(dims, np.float64)
    c = np.array(origin, np.float64) + 0.5 * ext
    m = float(ext.max())
    up = (0.0, 1.0, 0.0)
    if kind == "oblique":
        eye = c + 1.9 * m * np.array([-0.82, 0.41, 0.40])
    elif kind == "front":     # axis-aligned: with an odd frame size the centre row and column run exactly parallel to an axis
        eye = c + np.array([0.0, 0.0, 2.65 * m])
    elif kind == "above":     # axis-aligned and off the box: the centre row's rays are parallel to the xz plane ABOVE the box - the
        eye = c + np.array([0.0, 0.8 * ext[1], 1.4 * m])   # box test ignores that slab and they march outside the volume
        c = np.array([eye[0], eye[1], c[2]])
    elif kind == "inside":
        eye = c + ext * np.array([0.11, -0.07, 0.23])
    elif kind == "top":
        eye, up = c + np.array([0.0, 2.2 * m, 0.0]), (0.0, 0.0, -1.0)
    else:
        raise ValueError(kind)
    f32 = lambda v: np.array(v, dtype=np.float32)
    return f32(eye), f32(c), f32(up)


def _scene(name, dtype="f32", dims=(12, 12, 12), seed=1, vr=(0.0, 1.0), rate=1.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), cam="oblique", size=(20, 14),
           fovy=60.0, spp=1, frames=1, accumulate=False, sparse=0, tables=(16, 16, "ramp"), const_region=False):
    return dict(name=name, dtype=dtype, dims=dims, seed=seed, vr=vr, rate=rate, spacing=spacing, origin=origin, cam=cam, size=size, fovy=fovy, spp=spp, frames=frames,
                accumulate=accumulate, sparse=sparse, tables=tables, const_region=const_region)


# value ranges in the units the application passes them (integers for integer data).  The two 32-bit upper ends are the largest floats
# BELOW 2^32 / 2^31: the reference converts the float back with a plain cast, which is undefined at 2^32 / 2^31 themselves.
_FULL = {"u8": (0.0, 255.0), "i8": (-128.0, 127.0), "u16": (0.0, 65535.0), "i16": (-32768.0, 32767.0), "u32": (0.0, 4294967040.0),
         "i32": (-2147483648.0, 2147483520.0), "f32": (0.0, 1.0), "f64": (0.0, 1.0)}

SCENES = [
    # every voxel type over its full range (int8 / int32: the lower end is where integer_normalize clamps at -1)
    _scene("f32_oblique", "f32", (14, 12, 10), 1),
    _scene("u8_oblique", "u8", (12, 14, 10), 2, _FULL["u8"]),
    _scene("i8_oblique", "i8", (10, 12, 14), 3, _FULL["i8"]),
    _scene("u16_oblique", "u16", (12, 12, 12), 4, _FULL["u16"]),
    _scene("i16_oblique", "i16", (12, 10, 12), 5, _FULL["i16"]),
    _scene("u32_oblique", "u32", (12, 12, 10), 6, _FULL["u32"]),
    _scene("i32_oblique", "i32", (10, 12, 12), 7, _FULL["i32"]),
    _scene("f64_oblique", "f64", (12, 12, 12), 8),
    # value ranges inside / across the data range, per type (the table covers part of the data; samples outside clamp to its ends)
    _scene("f32_subrange", "f32", (12, 12, 12), 11, (0.25, 0.8), tables=(16, 16, "bumps")),
    _scene("u8_subrange", "u8", (12, 12, 12), 12, (40.0, 200.0), tables=(16, 16, "bumps")),
    _scene("i8_subrange", "i8", (12, 12, 12), 13, (-100.0, 90.0), tables=(16, 16, "sparse")),
    _scene("u16_subrange", "u16", (12, 12, 12), 14, (9000.0, 52000.0), tables=(16, 16, "bumps")),
    _scene("i16_subrange", "i16", (12, 12, 12), 15, (-20000.0, 25000.0), tables=(16, 16, "sparse")),
    _scene("u32_subrange", "u32", (12, 12, 12), 16, (500000000.0, 3500000000.0), tables=(16, 16, "bumps")),
    _scene("i32_subrange", "i32", (12, 12, 12), 17, (-1500000000.0, 1200000000.0), tables=(16, 16, "sparse")),
    _scene("f64_subrange", "f64", (12, 12, 12), 18, (0.3, 0.7), tables=(16, 16, "bumps")),
    _scene("f32_invalid_range", "f32", (12, 12, 12), 19, (1.0, -1.0)),   # an invalid range keeps the data range (volume.cpp:135-145)
    _scene("u8_invalid_range", "u8", (12, 12, 12), 20, (1.0, -1.0), tables=(16, 16, "sparse")),
    # sampling rates
    _scene("rate_half", "f32", (16, 16, 16), 21, rate=0.5, tables=(16, 16, "thin")),
    _scene("rate_4", "f32", (12, 12, 12), 22, rate=4.0, tables=(16, 16, "sparse"), size=(16, 12)),
    _scene("rate_4_u8", "u8", (12, 12, 12), 23, _FULL["u8"], rate=4.0, tables=(16, 16, "thin"), size=(16, 12)),
    _scene("rate_20", "f32", (8, 8, 8), 24, rate=20.0, tables=(16, 16, "sparse"), size=(12, 8)),
    # grids: anisotropic spacing, an origin off zero, the largest volume
    _scene("aniso_origin", "f32", (10, 14, 18), 25, spacing=(2.0, 1.0, 0.5), origin=(6.0, -3.5, 0.25)),
    _scene("aniso_origin_u16", "u16", (18, 10, 12), 26, _FULL["u16"], spacing=(0.5, 2.0, 1.0), origin=(-11.0, 4.0, 7.5), tables=(16, 16, "bumps")),
    _scene("aniso_rate4_i16", "i16", (10, 10, 16), 27, _FULL["i16"], rate=4.0, spacing=(1.0, 1.5, 0.75), origin=(1.0, 2.0, 3.0), size=(14, 10), tables=(16, 16, "sparse")),
    _scene("large_24", "f32", (24, 24, 24), 28, size=(24, 16), tables=(16, 16, "bumps")),
    # cameras: inside the box; axis-aligned with an odd frame size (ignored slab; rays marching outside the box)
    _scene("inside", "f32", (14, 14, 14), 29, cam="inside", fovy=90.0, tables=(16, 16, "thin")),
    _scene("inside_u8_aniso", "u8", (12, 16, 10), 30, _FULL["u8"], cam="inside", spacing=(1.0, 0.5, 2.0), origin=(3.0, 3.0, -9.0), tables=(16, 16, "sparse")),
    _scene("front_odd", "f32", (12, 12, 12), 31, cam="front", size=(21, 15), tables=(16, 16, "thin")),
    _scene("above_odd", "f32", (6, 6, 14), 32, cam="above", size=(15, 11), fovy=90.0, spacing=(2.0, 2.0, 0.5), origin=(6.0, 0.0, -3.5)),
    _scene("top_odd_i8", "i8", (12, 10, 12), 33, _FULL["i8"], cam="top", size=(17, 13), tables=(16, 16, "bumps")),
    # a constant region: zero gradient, NaN normal
    _scene("const_region", "f32", (12, 12, 16), 34, const_region=True, tables=(16, 16, "thin")),
    _scene("const_region_u8_front", "u8", (12, 12, 16), 35, _FULL["u8"], const_region=True, cam="front", size=(19, 13), tables=(16, 16, "thin")),
    # samples per pixel (TEA jitter), accumulation, a sparse frame
    _scene("spp3", "f32", (12, 12, 12), 36, spp=3, tables=(16, 16, "bumps")),
    _scene("spp3_accum3", "u8", (12, 12, 12), 37, _FULL["u8"], spp=3, frames=3, accumulate=True, size=(16, 12)),
    _scene("accum3", "f32", (12, 12, 12), 38, frames=3, accumulate=True, tables=(16, 16, "sparse")),
    _scene("frames3_no_accum", "f32", (12, 12, 12), 39, spp=3, frames=3, size=(16, 12)),
    _scene("sparse_list", "f32", (12, 12, 12), 40, sparse=70, size=(24, 16), tables=(16, 16, "bumps")),
    # table sizes
    _scene("tables_2_2", "f32", (12, 12, 12), 41, tables=(2, 2, "ramp")),
    _scene("tables_1024_1024", "f32", (12, 12, 12), 42, tables=(1024, 1024, "bumps")),
    _scene("tables_16_1024", "u8", (12, 12, 12), 43, _FULL["u8"], tables=(16, 1024, "sparse")),
    _scene("tables_1024_2", "f32", (12, 12, 12), 44, tables=(1024, 2, "ramp")),
    _scene("tables_2_16_u16", "u16", (12, 12, 12), 45, _FULL["u16"], tables=(2, 16, "bumps")),
]
# The condition on this list: both builds of the reference give equal counters on every scene.  A scene on which they disagree is
# replaced HERE, with a note, never exempted in a test (make_ref_march.py refuses to write the fixture otherwise).  Replacements so
# far: none - the list above is the first one tried.


def sparse_pixels(scene):
    """the pixel list of a sparse scene: `sparse` distinct pixels in row-major order (the order the reference's stream compaction keeps)"""
    w, h = scene["size"]
    idx = np.sort(np.random.default_rng(1000 + scene["seed"]).permutation(w * h)[: scene["sparse"]])
    return np.stack([idx % w, idx // w], axis=1).astype(np.int32)


def build_inputs(scene):
    vol = make_volume(scene["seed"], scene["dims"], scene["dtype"], scene["const_region"])
    colors, alphas = make_tables(*scene["tables"])
    eye, at, up = make_camera(scene["cam"], scene["dims"], scene["spacing"], scene["origin"])
    return dict(vol=vol, colors=colors, alphas=alphas, cam=(eye, at, up), pixels=sparse_pixels(scene) if scene["sparse"] else np.zeros((0, 2), np.int32),
                crc=zlib.crc32(np.ascontiguousarray(vol).tobytes()))


# ---- reading the fixture ---------------------------------------------------------------------------------------------------------------
QUANTITIES = ("alpha", "colour", "grad")


def quantities(rgba, grad):
    """what the comparisons look at: alpha, premultiplied colour, premultiplied gradient (the frame holds both divided by alpha, which is
    ill-conditioned where alpha is tiny) - float64"""
    rgba, grad = np.asarray(rgba, np.float32).astype(np.float64), np.asarray(grad, np.float32).astype(np.float64)
    a = rgba[..., 3]
    return {"alpha": a, "colour": rgba[..., :3] * a[..., None], "grad": grad * a[..., None]}


def load_fixture(path):
    """-> (scenes, D): one dict per scene (the parameters of SCENES plus vol, colors, alphas, cam, pixels, rgba / grad of both builds as float32,
    counters (primary, shadow)); D[q] = the largest difference between the reference's two builds over ALL scenes, per quantity"""
    import json
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    scenes, D = [], {q: 0.0 for q in QUANTITIES}
    for i, m in enumerate(meta):
        k = f"s{i:02d}_"
        s = dict(m)
        s["vol"] = make_volume(m["seed"], m["dims"], m["dtype"], m["const_region"])
        assert zlib.crc32(np.ascontiguousarray(s["vol"]).tobytes()) == m["crc"], f"{m['name']}: the regenerated volume is not the one the reference was fed"
        s["colors"], s["alphas"], s["pixels"] = z[k + "colors"], z[k + "alphas"], z[k + "pixels"]
        cam = z[k + "cam"]
        s["cam_kind"], s["cam"] = m["cam"], (cam[0:3], cam[3:6], cam[6:9])
        for tag in ("", "_fma"):
            s["rgba" + tag], s["grad" + tag] = z[k + "rgba" + tag].view(np.float32), z[k + "grad" + tag].view(np.float32)
        s["basis"] = z[k + "basis"]   # the launch parameters' camera: position, direction, horizontal, vertical (float32, the reference's host math)
        c = z[k + "counters"]
        assert (c[0] == c[1]).all(), f"{m['name']}: the two builds of the reference disagree about a count - the scene must be replaced"
        s["primary"], s["shadow"] = int(c[0, 0]), int(c[0, 1])
        qa, qb = quantities(s["rgba"], s["grad"]), quantities(s["rgba_fma"], s["grad_fma"])
        for q in QUANTITIES:
            D[q] = max(D[q], float(np.abs(qa[q] - qb[q]).max()))
        scenes.append(s)
    return scenes, D


def band_excess(scene, D, rgba, grad, factor=4.0, cap=None, which=QUANTITIES, pixels=None):
    """How far `rgba` / `grad` lie outside the band around the reference's frames, per quantity: the element-wise distance to the NEARER of the
    two builds must not exceed factor * D[q] (two float32 steps at the value's magnitude, should D[q] be 0), nor `cap` if given.
    -> {q: (largest distance, tolerance there, largest distance / tolerance)}; within the band iff every ratio is <= 1."""
    got = quantities(rgba, grad)
    qa, qb = quantities(scene["rgba"], scene["grad"]), quantities(scene["rgba_fma"], scene["grad_fma"])
    out = {}
    for q in which:
        g, a, b = got[q], qa[q], qb[q]
        if pixels is not None:   # a sparse frame: only the listed pixels were rendered
            sel = (pixels[:, 1], pixels[:, 0])
            g, a, b = g[sel], a[sel], b[sel]
        dist = np.minimum(np.abs(g - a), np.abs(g - b))
        tol = np.full(dist.shape, factor * D[q]) if D[q] > 0 else 2.0 * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
        if cap is not None:
            tol = np.minimum(tol, cap)
        dist = np.where(np.isnan(dist), np.inf, dist)   # a NaN where the reference has a number is outside any band
        dist = np.where(np.isnan(a) & np.isnan(b) & np.isnan(g), 0.0, dist)
        i = int(np.argmax(dist / tol))
        out[q] = (float(dist.ravel()[i]), float(tol.ravel()[i]), float((dist / tol).ravel()[i]))
    return out
