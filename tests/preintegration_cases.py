"""Inputs shared by tests/test_preintegration_model.py (no GPU) and tests/test_preintegration_gpu.py: the volumes, the transfer functions and the committed case
of the pre-integration tests (include/ovr_hip.h ovr_hip_set_preintegration).  Image size, cameras, rays and the random / smooth volumes are projection_cases'
(signed_cases' for the signed type); the borderline cap is slice_context_cases'.

THE COMMITTED CASE (model test 5 and the GPU frames): the `smooth` volume (a blob plus 5 % noise) under the `ones` transfer function - 16 entries, alpha
min(1, 6 i / 15), so every entry from the third on is exactly 1 - over the type's whole range, the axis camera, sampling rate 1.  The node table then has 61
nodes: the noise moves the coordinate by less than a node per step outside the blob (rays of first-branch segments alone) and by more on its flanks (integral
segments), the blob saturates the rays through it and the noise floor leaves partial ones.  How it was chosen: a ray nears the termination threshold 0.9999
in increments of any size, and of the slopes 1.2 ... 10, the rates 0.5, 1 and 2.7 and the two cameras most combinations leave 1 - 3 % of the hit rays with a loop
test within 1e-5 of it; this one leaves 2 of 572 for every voxel type (tests/test_preintegration_model.py asserts the classes and the cap)."""
import numpy as np

import projection_cases as PC
import signed_cases as SG
from slice_context_cases import BORDER_CAP

F = np.float32
ERT = F(0.9999)
RATE = 1.0
RATES = (0.5, 1.0, 2.7)
CAMERA = "axis"
TF = "ones"
VOLUME = "smooth"
DTYPES = PC.DTYPES + (np.int16,)
TFS = ("dense", "shell", "ones")
BORDER = 1e-5        # a ray is borderline when a loop test met an alpha this close to ERT
DU_BORDER = 1e-4     # ... or, for 8-bit voxels, a segment whose fabs(du) * (M - 1) lies this close to 1
__all__ = ["BORDER_CAP"]


def volume(kind, dtype, dims=PC.DIMS[0]):
    return SG.volume(kind, dtype, dims) if SG.is_signed(dtype) else PC.volume(kind, dtype, dims)


def constant_volume(dtype, dims=PC.DIMS[0]):
    """every voxel equal: 0.4 of the type's positive range"""
    nx, ny, nz = dims
    dt = np.dtype(dtype)
    v = 0.4 if dt.kind == "f" else int(0.4 * np.iinfo(dt).max)
    return np.full((nz, ny, nx), v, dt)


def ramp_volume(dims=PC.DIMS[0], lo=0.1, hi=0.9):
    """float32, a linear ramp along z from lo at the first voxel centre to hi at the last one; constant across x and y"""
    nx, ny, nz = dims
    z = lo + (hi - lo) * np.arange(nz, dtype=np.float64) / (nz - 1)
    return np.ascontiguousarray(np.broadcast_to(z[:, None, None], (nz, ny, nx)).astype(F))


def value_range(dtype, volume_kind):
    dt = np.dtype(dtype)
    if dt == np.float32:
        return (-0.5, 0.5) if volume_kind == "random" else (0.0, 1.0)
    return (float(np.iinfo(dt).min), float(np.iinfo(dt).max))   # the type's whole range (signed_cases shifts the field by the type's minimum)


def transfer_function(ovr, kind, dtype, volume_kind=VOLUME):
    """(colors flat 3 n, alphas flat (pos, alpha) 2 n, value_range).  dense: 16 entries, alpha 0.9 i / 15; shell: 64 entries, zero but for two peaks two
    entries wide (a thin shell: narrower than the data's change over a step); ones: 16 entries, alpha min(1, 6 i / 15) - entries that are exactly 1"""
    n = 64 if kind == "shell" else 16
    colors, alphas, _ = ovr.synth.make_tfn("dense", n, dtype)
    alphas = np.array(alphas, F).copy()
    i = np.arange(n, dtype=np.float64)
    if kind == "shell":
        a = np.zeros(n)
        a[20:22] = 0.85
        a[41:43] = 0.6
    elif kind == "ones":
        a = np.minimum(1.0, 6.0 * i / (n - 1))
    elif kind == "dense":
        a = 0.9 * i / (n - 1)
    else:
        raise ValueError(kind)
    alphas[1::2] = a.astype(F)
    return colors, alphas, value_range(dtype, volume_kind)


def classes(r):
    """the model's rays (preintegration.preintegrated_rays) by class"""
    a = r["rgba"][:, 3]
    taken = r["steps"] > 0
    return dict(first_only=taken & (r["integral"] == 0), integral=r["integral"] > 0, saturated=taken & (a >= ERT), partial=taken & (a > 0) & (a < ERT))
