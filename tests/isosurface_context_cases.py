"""Inputs shared by tests/test_isosurface_context_model.py (no GPU) and tests/test_isosurface_context_gpu.py: the volumes, level sets and transfer functions of the
isosurface-context tests (include/ovr_hip.h ovr_hip_set_isosurface_context).  Volumes, image size, cameras and rays are projection_cases' and isosurface_cases'
(signed_cases' for the signed type).

THE COMMITTED CASE: the `ball` volume (value = clamp(1 - r / R) around the centre: its level sets are nested spheres, so that a ray through the middle meets
events 0, 1, 1, 0), the two outer levels of isosurface_cases.NESTED with the opacities SHELLS, the "dense" transfer function (alpha 0.9 i / (n - 1)) over the
type's whole range, the axis camera, sampling rate 0.5 - slice_context_cases' reasoning: with the doubled step the opacity correction squares the transparency
per step, a ray nears the termination threshold 0.9999 in large increments and few rays end within 1e-5 of it.  Among the two cameras, the rates 0.5 / 1 and
the level pairs of NESTED this one gives the most rays with an event (76 of 1120) and no borderline ray on the float32 volume at either scale; the oblique
camera at rate 1 has 11 of 60 (tests/test_isosurface_context_model.py asserts the cap for every type and both scales)."""
import numpy as np

import isosurface_cases as IC
import projection_cases as PC
import signed_cases as SG

F = np.float32
KIND = "ball"
LEVELS = IC.NESTED["ball"][0:2]     # fractions of full scale: 0.2, 0.35
SHELLS = (0.4, 0.6)                 # their opacities: nested translucent shells
OPAQUE_LEVEL = (IC.NESTED["ball"][2],)
UNREACHABLE = (5.0, 7.0)            # fractions of full scale above every sample of every type
RATE = 0.5
CAMERA = "axis"
SCALES = (1.0, 0.3)
ERT = F(0.9999)
BORDER = 1e-5           # a ray is borderline when the model's A in front of an event or a step lies this close to ERT
BORDER_CAP = 0.01       # the share of the rays with an event the product-build comparison may leave out
DTYPES = PC.DTYPES + (np.int16,)
CLIP = ((5.5, -float("inf"), 3.0), (27.0, 20.25, float("inf")))


def volume(dtype, dims=PC.DIMS[0], kind=KIND):
    return SG.any_volume(kind, dtype, dims)


def isovalues(fractions, dtype):
    return SG.any_scaled(fractions, dtype)


def transfer_function(ovr, kind, dtype, n=16):
    """(colors flat 3 n, alphas flat (pos, alpha) 2 n, value_range): `dense` over the type's whole range; `zero`: the same colours under an all-zero alpha table"""
    colors, alphas, vr = ovr.synth.make_tfn("dense", n, dtype)
    alphas = np.array(alphas, F).copy()
    if kind == "zero":
        alphas[1::2] = 0.0
    elif kind != "dense":
        raise ValueError(kind)
    return colors, alphas, vr
