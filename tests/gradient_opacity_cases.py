"""Inputs shared by tests/test_gradient_opacity_model.py (no GPU) and tests/test_gradient_opacity_gpu.py: the volumes, the ramps and the committed case of the
gradient-opacity tests (include/ovr_hip.h ovr_hip_set_gradient_opacity).  Image size, cameras, rays, the smooth volume and the transfer functions are
projection_cases' and preintegration_cases'.

THE COMMITTED CASE (the model's cap test and the GPU frames): the `smooth` volume (a blob plus 5 % noise, 40 x 33 x 18) under the `ones` transfer function over
the type's whole range, the axis camera, sampling rate 1, the ramp (0.02, 0.06): the 5th and the 60th percentile, roughly, of the volume's magnitudes
(gradient_opacity.magnitudes: 0.017 ... 0.107 between the 5th and the 95th).  The blob's flanks saturate the rays through them, the noise floor leaves partial
ones; 5 - 7 of the 572 hit rays have a loop test within 1e-5 of 0.9999 for every voxel type (the cap is 1 in 50; the oblique camera and the ramp (0.03, 0.08)
leave 11 of 406, over it: not chosen)."""
import numpy as np

import preintegration_cases as QC
import projection_cases as PC

F = np.float32
OFF, RAMP = 0, 1
NEUTRAL = (-1.0, 0.0)      # w == 1 for every m >= 0
VOLUME, TF, CAMERA, RATE = "smooth", "ones", "axis", 1.0
RAMP_CASE = (0.02, 0.06)
BORDER = 1e-5              # a ray is borderline when a loop test met an alpha this close to 0.9999
W_BORDER = 1e-4            # a gradient step is borderline when (m - lo) * inv_ramp lies this close to 0
BORDER_CAP = 1.0 / 50.0    # the share of the hit rays that may be borderline
LIGHT = (0.3, -1.0, 0.55)                  # not the reference's
MATERIAL = (0.35, 0.7, 0.45, 12.0)         # ambient, diffuse, specular, shininess: a specular material
INTENSITY = 1.25
# consequence 2: a 16^3 f32 ramp v = x / 32 under the range [0, 0.5] and the ramp (0, 0.125), cut to [3, 13]^3 so that no sample lies in the clamp-to-edge
# half voxels: every gradient is exactly (1/32, 0, 0), m = 1/16 and w = 0.5
RAMP_DIMS = (16, 16, 16)
RAMP_RANGE = (0.0, 0.5)
RAMP_HALF = (0.0, 0.125)
RAMP_CLIP = ((3.0, 3.0, 3.0), (13.0, 13.0, 13.0))
RAMP_SATURATED = (-1.0, 1.0 / 32.0)        # consequence 4: hi at half the slope (m = 1/16), so that w == 1 whatever the rounding of m


def x_ramp_volume():
    """float32 16^3, v = x / 32 at voxel x (exact)"""
    nx, ny, nz = RAMP_DIMS
    x = (np.arange(nx, dtype=np.float64) / 32.0).astype(F)
    return np.ascontiguousarray(np.broadcast_to(x[None, None, :], (nz, ny, nx)).astype(F))


def step_volume():
    """float32 16^3: 0.25 below x = 8, 0.75 from there on - two homogeneous materials and one boundary"""
    nx, ny, nz = RAMP_DIMS
    x = np.where(np.arange(nx) < 8, 0.25, 0.75).astype(F)
    return np.ascontiguousarray(np.broadcast_to(x[None, None, :], (nz, ny, nx)).astype(F))


def ramp_tables(ovr, half=False):
    """the dense table (16 entries, alpha 0.9 i / 15) over RAMP_RANGE; half: its alphas times 0.5 (exact)"""
    colors, alphas, _ = QC.transfer_function(ovr, "dense", np.float32)
    alphas = np.array(alphas, F).copy()
    if half:
        alphas[1::2] = (alphas[1::2] * F(0.5)).astype(F)
    return colors, alphas, RAMP_RANGE


def dyadic_rays():
    """rays with dyadic origins (multiples of 0.5) along (0, 0, 1), (1, 0, 0) and (1, 0, 1) through the 16^3 box, started outside it: (org, dir), each (n, 3)"""
    org, d = [], []
    for a in np.arange(3.5, 13.0, 1.5):
        for b in np.arange(4.0, 13.0, 2.5):
            org.append((a, b, -4.0)); d.append((0.0, 0.0, 1.0))
            org.append((-4.0, a, b)); d.append((1.0, 0.0, 0.0))
            org.append((a - 12.0, b, -8.0)); d.append((1.0, 0.0, 1.0))
    return np.array(org, F), np.array(d, F)


def case_tables(ovr, dtype, tf=TF, volume_kind=VOLUME):
    colors, alphas, vr = QC.transfer_function(ovr, tf, dtype, volume_kind)
    ct, at = PC.tables(colors, alphas)
    return (colors, alphas, vr), ct, at, ovr.projection.normalized_range(vr, dtype)
