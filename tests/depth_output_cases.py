"""Inputs shared by tests/test_depth_output_model.py (no GPU) and tests/test_depth_output_gpu.py: the thresholds, the committed case and the seeded rays of the
depth-layer tests (include/ovr_hip.h ovr_hip_set_depth_output).  Everything else is max_depth_cases', projection_cases' and gradient_opacity_cases': the
`smooth` 40 x 33 x 18 volume, the 16^3 ramp, their image size and cameras, the tilted plane, the light and the material.

THE COMMITTED CASE (the model's identities and cap test, the GPU frames against the model): max_depth_cases' - the `smooth` volume under the `ones` transfer
function over the type's whole range, the axis camera, sampling rate 1 - with no depth image, or with max_depth_cases.plane_image."""
import numpy as np

import gradient_opacity_cases as GC
import max_depth_cases as MC
import projection_cases as PC

F = np.float32
TAU_FIRST = float(np.finfo(F).tiny)      # the smallest positive normal float: the back end of the first step with opacity
TAUS = (TAU_FIRST, 0.25, 0.5, 0.9)       # the model's identities
GPU_TAUS = (TAU_FIRST, 0.5)              # the GPU comparison against the model
VOLUME, TF, CAMERA, RATE = MC.VOLUME, MC.TF, MC.CAMERA, MC.RATE
BORDER, BORDER_CAP = MC.BORDER, MC.BORDER_CAP
LIGHT, MATERIAL, INTENSITY = MC.LIGHT, MC.MATERIAL, MC.INTENSITY
SIZE = PC.SIZE
NOISE_SEED = 77                          # the blue-noise tile of the jittered frames: max_depth's


def seeded_rays():
    """max_depth_cases.seeded_rays: (org, dir, depth) - the same rays run with their depths and without"""
    return MC.seeded_rays()


SHORT_CHORD = 14.0


def short_chord_rays(ovr):
    """the seeded rays for the run WITHOUT depths: those that miss the box or cross at most SHORT_CHORD of it.  Run to t1 under the `ones` table every second
    seeded ray saturates, and about 6 in 100 saturating rays meet a loop test within BORDER of 0.9999 - 77 of the 2114 hit rays, over the cap of 1 in 50 (the
    model test prints it); the seeded depths cut most of those rays short, a short chord does the same without a depth: 3 of 289 hit rays"""
    org, d, _ = MC.seeded_rays()
    inv, wp = ovr.clipping.volume_constants(PC.DIMS[0])
    t0, t1, hit = ovr.clipping.world_intervals(org, d, inv, wp, (0, 0, 0), (1, 1, 1))
    keep = ~hit | ((t1 - t0) <= F(SHORT_CHORD))
    return org[keep], d[keep]


def noise_tile():
    return np.random.default_rng(NOISE_SEED).random((16, 16, 64)).astype(F)


def ramp_volume_and_tables(ovr):
    return MC.ramp_volume_and_tables(ovr)


def dyadic_rays():
    return GC.dyadic_rays()


def constant_volume(value=0.5, dims=(16, 16, 16)):
    """a volume of one value: every step of a ray has the same corrected opacity (but a shortened last one)"""
    return np.full(dims[::-1], value, F)
