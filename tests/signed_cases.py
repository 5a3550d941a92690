"""Inputs shared by tests/test_signed_types_model.py (no GPU), tests/test_signed_types_gpu.py and tests/test_addressing_matrix_gpu.py: the volumes of
projection_cases and isosurface_cases as int8 and int16, their isovalues in the samples' units, a float64 restatement of the signed tap and the addressing
settings the GPU files walk.  Dimensions, image size, rays, cameras and tables stay projection_cases': the x sizes 40 and 24 meet every pair position of a
4-voxel (16-bit) and an 8-voxel (8-bit) brick row, and no axis is a multiple of a brick or a cell.  Everything is cached and read-only."""
import numpy as np

import isosurface_cases as IC
import projection_cases as PC

F = np.float32
DIMS, SIZE, RATES, CAMERAS, FOVY = PC.DIMS, PC.SIZE, PC.RATES, PC.CAMERAS, PC.FOVY
DTYPES = (np.int8, np.int16)
UNSIGNED = {np.dtype(np.int8): np.uint8, np.dtype(np.int16): np.uint16}
MINIMUM = {np.dtype(np.int8): -128, np.dtype(np.int16): -32768}
ROWS = {"OVR_HIP_ROW_LOADS": "1"}       # the aligned 8-byte row loads of the 16- and 8-bit layouts: addressing mode 4 (csrc/host/launch_plan.hpp)
ADDRESSING = (0, 1, 2, 3, "rows")       # OVR_HIP_ADDRESSING = 0 ... 3, or ROWS and no override
# isovalues in the samples' units (int8: normalised by 1 / 127 behind the clamp of -128 to -127; int16: raw)
INT8_EDGES = {
    "clamp": F(-126.5 / 127.0),     # separates the voxels -128 and -127 (both -1.0 behind the clamp) from -126
    "all_minimum": F(-1.0),         # every sample is on or above it: no ray changes side
    "zero": F(0.0),
}
INT16_EDGES = {"zero": F(0.0), "half": F(-0.5), "low": F(-20000.25)}      # (low: below -2^14)
EDGES = {np.dtype(np.int8): INT8_EDGES, np.dtype(np.int16): INT16_EDGES}
_cache = {}


def volume(kind, dtype, dims=DIMS[0]):
    """the field of the same kind (projection_cases' kinds and isosurface_cases' `ball`), quantised like its unsigned twin and shifted by the type's minimum: the
    exterior of `ball` and whatever quantises to 0 are the type's minimum"""
    dt = np.dtype(dtype)
    key = (kind, dt.name, tuple(dims))
    if key not in _cache:
        u = IC.volume(kind, UNSIGNED[dt], dims)
        _cache[key] = PC._frozen(np.ascontiguousarray((u.astype(np.int32) + MINIMUM[dt]).astype(dt)))
    return _cache[key]


def minimum_blocks(dtype, dims=DIMS[0], seed=19):
    """a random volume over the type's whole range holding blocks of the type's minimum next to minimum + 1: the clamp's two inputs side by side"""
    dt = np.dtype(dtype)
    key = ("minimum_blocks", dt.name, tuple(dims), seed)
    if key not in _cache:
        nx, ny, nz = dims
        rng = np.random.default_rng([seed, nx, ny, nz])
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max + 1, (nz, ny, nx)).astype(dt)
        v[2:9, 3:12, 5:17] = info.min
        v[2:9, 3:12, 17:23] = info.min + 1
        v[4:7, 12:15, 5:23] = np.where(rng.random((3, 3, 18)) < 0.5, info.min, info.min + 1).astype(dt)
        _cache[key] = PC._frozen(v)
    return _cache[key]


def scaled(fractions, dtype):
    """isovalues given as fractions of the unsigned twin's full scale, in the units of the signed type's samples; float32, ascending"""
    f = np.asarray(fractions, np.float64)
    v = (f * 255.0 - 128.0) / 127.0 if np.dtype(dtype) == np.int8 else f * 65535.0 - 32768.0
    return np.sort(v.astype(F))


def values64(volume):
    """the voxels in the samples' units, float64: int8 as max(v / 127, -1), int16 raw"""
    v = np.asarray(volume)
    return np.maximum(v.astype(np.float64) / 127.0, -1.0) if v.dtype == np.int8 else v.astype(np.float64)


def sample64(volume, po):
    """isosurface_cases.sample64 over values64: the trilinear field of a signed volume in float64"""
    return IC.sample64(values64(volume), po)


def root64(volume, org, direction, ta, tb, iso):
    """isosurface_cases.root64 over values64"""
    return IC.root64(values64(volume), org, direction, ta, tb, iso)


def clamp_isovalues():
    """the clamp case's isovalues (int8 `ball`): two nested levels and the one between the clamped voxels and -126"""
    return np.sort(np.concatenate([scaled(IC.NESTED["ball"][1:3], np.int8), [INT8_EDGES["clamp"]]]).astype(F))


def layer_isovalues(dtype):
    """four nested isovalues of `ball` for the translucent and the AO walks: isosurface_cases.NESTED, its outermost level replaced by the signed type's lowest edge
    (int8: the level between the clamped voxels and -126, met where the exterior's -128 begins; int16: the one below -2^14)"""
    if not is_signed(dtype):
        return IC.scaled(IC.NESTED["ball"], dtype)
    lowest = INT8_EDGES["clamp"] if np.dtype(dtype) == np.int8 else INT16_EDGES["low"]
    return np.sort(np.concatenate([[lowest], scaled(IC.NESTED["ball"][1:], dtype)]).astype(F))


# the frames of the GPU files: the oblique camera at rate 2.5, the image 40 x 28
CAMERA, FRAME_RATE = "oblique", 2.5
MIXED = (0.3, 0.4, 0.5, 1.0)
AO = (3, 6.0)                           # K, R of the AO frames (under gradient shading)
PROJECTION_KINDS = ("random",)
SKIPPING_KINDS = ("slab", "plateau", "ball")      # (`ball`: cells that hold the type's minimum alone)


def iso_frames(dtype):
    """name -> (volume kind, isovalues ascending, opacities or None) of every isosurface frame case the GPU files draw"""
    dt = np.dtype(dtype)
    edge = clamp_isovalues() if dt == np.int8 else np.sort(np.array(list(INT16_EDGES.values()), F))
    out = {
        "opaque": ("ball", scaled(IC.NESTED["ball"][:2], dt), None),
        "edge": ("ball", edge, None),
        "translucent": ("ball", layer_isovalues(dt), MIXED),
    }
    for kind in SKIPPING_KINDS:
        out[kind] = (kind, scaled(IC.ISOVALUES[kind], dt), None)
    return out


def environment(am):
    """the variables one entry of ADDRESSING sets; None: neither (the mode the layout's size asks for), "no rows": the row loads forced off"""
    if am is None:
        return {}
    if am == "rows":
        return dict(ROWS)
    if am == "no rows":
        return {"OVR_HIP_ROW_LOADS": "0"}
    return {"OVR_HIP_ADDRESSING": str(am)}


def set_addressing(monkeypatch, am):
    """OVR_HIP_ROW_LOADS is read when a renderer is created, OVR_HIP_ADDRESSING with every launch plan: call this BEFORE hip_renderer_factory() and keep it for
    the renderer's life.  An override above 0 would keep mode 4 away (plan_addressing), so "rows" removes it"""
    for name in ("OVR_HIP_ADDRESSING", "OVR_HIP_ROW_LOADS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in environment(am).items():
        monkeypatch.setenv(name, value)


# the unsigned twins through the same names: the addressing matrix walks uint16 and uint8 with the signed files' bodies
def is_signed(dtype):
    return np.dtype(dtype) in MINIMUM


def any_volume(kind, dtype, dims=DIMS[0]):
    if is_signed(dtype):
        return minimum_blocks(dtype, dims) if kind == "random" else volume(kind, dtype, dims)
    return IC.volume(kind, dtype, dims)


def any_scaled(fractions, dtype):
    return scaled(fractions, dtype) if is_signed(dtype) else IC.scaled(fractions, dtype)


def edge_isovalues(dtype):
    """three isovalues for the opaque known-answer entry and the `edge` frames: the type's named edges where it has some"""
    return iso_frames(dtype)["edge"][1] if is_signed(dtype) else IC.scaled(IC.NESTED["ball"][1:], dtype)
