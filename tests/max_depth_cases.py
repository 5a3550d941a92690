"""Inputs shared by tests/test_max_depth_model.py (no GPU) and tests/test_max_depth_gpu.py: the depth images, the clip boxes and the committed case of the
depth-limit tests (include/ovr_hip.h ovr_hip_set_max_depth).  Image size, cameras, the smooth volume and the transfer functions are projection_cases',
preintegration_cases' and gradient_opacity_cases'.

THE COMMITTED CASE (the model's cap test and the GPU frames against the model): the `smooth` volume (40 x 33 x 18) under the `ones` transfer function over the
type's whole range, the axis camera, sampling rate 1, and plane_image: a tilted plane of ray parameters through the volume - the axis camera stands 60 world
units in front of the box, whose rays run from t of about 60 to about 79 - with a disc of +inf (no surface: those rays run to t1) and a patch of NaN (likewise)."""
import numpy as np

import gradient_opacity_cases as GC
import preintegration_cases as QC
import projection_cases as PC

F = np.float32
INF = float("inf")
VOLUME, TF, CAMERA, RATE = GC.VOLUME, GC.TF, GC.CAMERA, GC.RATE
BORDER, BORDER_CAP = GC.BORDER, GC.BORDER_CAP
LIGHT, MATERIAL, INTENSITY = GC.LIGHT, GC.MATERIAL, GC.INTENSITY
CENTRE = (20.0, 16.5, 9.0)
ORTHO_EYE = (-31.5, 44.25, -39.0)      # the oblique camera's eye
ORTHO_HEIGHT = 40.0
# a clip box for the `no surface` identity: cuts on every axis
CLIP = ((5.5, -INF, 3.0), (27.0, 20.25, INF))
# depth = crop: seen from the oblique eye (the viewing direction is (+, -, +)) the far sides of the box are +x, -y and +z; this box removes only those
FAR_CLIP = ((-INF, 8.0, -INF), (27.0, INF, 12.0))
CROP_SIZES = ((37, 23), (56, 40))      # no multiples of the 8 x 8 block
# the tilted plane of the committed case under the axis camera: t = PLANE[0] + PLANE[1] * ix + PLANE[2] * iy
PLANE = (61.0, 0.32, 0.21)
# the orthographic twin, from the oblique eye: the rays run from t of about 45 to about 110
ORTHO_PLANE = (60.0, 0.55, 0.4)


def plane_image(size=PC.SIZE, plane=PLANE):
    """(H, W) float32: the tilted plane, a disc of +inf around (0.3 W, 0.6 H) and a patch of NaN in the upper right"""
    w, h = size
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = (plane[0] + plane[1] * ix + plane[2] * iy).astype(F)
    z[(ix - 0.3 * w) ** 2 + (iy - 0.6 * h) ** 2 <= (0.17 * h) ** 2] = np.inf
    z[h // 8:h // 8 + max(h // 5, 2), (5 * w) // 8:(5 * w) // 8 + max(w // 6, 2)] = np.nan
    return z


def no_surface_images(size, t1_max):
    """the three images that put no surface anywhere: +inf, NaN, and a value at or above every t1"""
    w, h = size
    return {"inf": np.full((h, w), np.inf, F), "nan": np.full((h, w), np.nan, F), "beyond": np.full((h, w), np.nextafter(F(t1_max), F(np.inf)), F)}


def case_tables(ovr, dtype, tf=TF, volume_kind=VOLUME):
    return GC.case_tables(ovr, dtype, tf, volume_kind)


def ramp_volume_and_tables(ovr):
    """the 16^3 ramp of gradient_opacity_cases under the halved dense table: alphas of at most 0.45, so that a ray of a few steps does not saturate"""
    colors, alphas, vr = GC.ramp_tables(ovr, True)
    return GC.x_ramp_volume(), colors, alphas, vr


def seeded_rays(n=2400, seed=26):
    """world rays towards the 40 x 33 x 18 box from all around it, one in eight misses, and a depth per ray: most inside the volume (the box's centre lies at
    t = 70), some +inf, NaN, in front of the ray's origin.  (org, dir, depth); 31 - 32 of the 2114 hit rays have a loop test within BORDER of 0.9999 (the cap is
    1 in 50; depths spread over 45 ... 95 leave 47 - 50, over it: not chosen)"""
    rng = np.random.default_rng(seed)
    dims = np.array(PC.DIMS[0], np.float64)
    target = rng.random((n, 3)) * dims
    target[::8] += 3.0 * dims      # misses
    v = rng.normal(size=(n, 3))
    org = 0.5 * dims + 70.0 * v / np.linalg.norm(v, axis=1)[:, None]
    d = target - org
    z = (50.0 + 30.0 * rng.random(n)).astype(F)
    z[3::11] = np.inf
    z[5::13] = np.nan
    z[7::17] = -2.0
    return org.astype(F), (d / np.linalg.norm(d, axis=1)[:, None]).astype(F), z


STEP_KS = (1, 2, 3)      # depth = t0 + k * step on the dyadic rays
