"""Inputs shared by tests/test_slice_context_model.py (no GPU) and tests/test_slice_context_gpu.py: the slice sets, the transfer functions and the committed
case of the slice-context tests (include/ovr_hip.h ovr_hip_set_slice_context).  Volumes, image size, cameras and rays are projection_cases' (signed_cases' for
the signed type).

THE COMMITTED CASE (model test 4 and GPU test 4): the `random` volume, the "dense" transfer function (alpha 0.9 i / (n - 1)) over the data's whole range, the
oblique camera, SLICES - a plane and a 3-voxel MAXIMUM slab through the centre - at sampling rate 0.5.  How it was chosen: with opacities of 0.2 ... 0.5 per
step a ray approaches the termination threshold 0.9999 in increments of a few 1e-5, and every fifth saturating ray ends within 1e-5 of it - far above the 1 %
of the met rays that the product-build comparison may leave out.  Rate 0.5 doubles the step, the opacity correction squares the transparency per step and the
increments grow; among the plane / slab orientations through the centre that give every class at least 25 rays this one has the fewest borderline rays
(2 of 290 met on the float32 volume; tests/test_slice_context_model.py asserts the cap)."""
import numpy as np

import projection_cases as PC
import signed_cases as SG

F = np.float32
MAXIMUM, MINIMUM, MEAN = 1, 2, 3
CENTRE = (20.0, 16.5, 9.0)
SLICES = [(CENTRE, (-0.1, -0.4, 1.0)), (CENTRE, (0.3, -0.6, -1.3), 3.0, MAXIMUM)]
RATE = 0.5
CAMERA = "oblique"
# slices that no ray of either camera meets: a plane and a slab far outside the box
NO_MEET = [((1000.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((0.0, -500.0, 0.0), (0.0, 1.0, 0.0), 3.0, MEAN)]
# the slice sets of the known-answer test: a plane, plane + slabs, a thin slab
SETS = {
    "case": SLICES,
    "plane": [(CENTRE, (1.0, 2.0, -1.0))],
    "plane+slab": [((14.0, 20.0, 6.0), (2.0, -1.0, 3.0)), ((25.0, 10.0, 12.0), (-1.0, 1.0, 2.0), 4.0, MEAN), ((8.0, 8.0, 8.0), (3.0, 1.0, 1.0), 6.0, MINIMUM)],
    "thin": [(CENTRE, (1.0, 2.0, -1.0), 0.25, MAXIMUM)],
    "no meet": NO_MEET,
}
ERT = F(0.9999)
BORDER = 1e-5           # a ray is borderline when the model's alpha before the slice lies this close to ERT
BORDER_CAP = 0.01       # the share of the met rays the product-build comparison may leave out
DTYPES = PC.DTYPES + (np.int16,)


def volume(dtype, dims=PC.DIMS[0]):
    return SG.volume("random", dtype, dims) if SG.is_signed(dtype) else PC.volume("random", dtype, dims)


def transfer_function(ovr, kind, dtype, n=16):
    """(colors flat 3 n, alphas flat (pos, alpha) 2 n, value_range): `dense` over the whole range of the `random` volume of the type; `zero`: the same colours
    under an all-zero alpha table"""
    colors, alphas, vr = ovr.synth.make_tfn("dense", n, dtype)
    if np.dtype(dtype) == np.float32:
        vr = (-0.5, 0.5)   # the shifted random volume's range
    alphas = np.array(alphas, F).copy()
    if kind == "zero":
        alphas[1::2] = 0.0
    elif kind != "dense":
        raise ValueError(kind)
    return colors, alphas, vr


def classes(r):
    """the model's rays (slice_context.context_rays) by class: saturated before the slice, slice composited behind a partial alpha, no slice met but marched;
    and the borderline rays among the met ones"""
    af = r["alpha_front"]
    return dict(saturated=r["met"] & (af >= ERT), partial=(r["k"] > 0) & (af > 0) & (af < ERT), unmet=~r["met"] & (r["steps"] > 0),
                borderline=r["met"] & (np.abs(af.astype(np.float64) - float(ERT)) <= BORDER))   # (r["borderline"]: the same test at every step of every ray)
