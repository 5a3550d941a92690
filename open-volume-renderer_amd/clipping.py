"""The clip box of the HIP backend (include/ovr_hip.h, ovr_hip_set_clip_box) as a numpy model: the normative text.

World box: `lower[3]`, `upper[3]` in the space of grid_origin / grid_spacing; lower may hold -inf, upper +inf ("open on
this side").

Object box: the kernels march in the volume's object space, where the volume is the unit cube.  A world position p becomes
fma(p, inv_scale, wto_p) per axis (`to_object`), with the float32 constants the host derives from the volume
(`volume_constants`):

    ext = n (cell-centred grid) or n - 1 (vertex-centred);  inv_scale = 1 / (spacing * ext);  wto_p = -(inv_scale * origin)

and the clip box becomes, per axis,

    lo = clamp01(fma(lower, inv_scale, wto_p))      hi = clamp01(fma(upper, inv_scale, wto_p))

(-inf -> 0, +inf -> 1; clamp01(x) = fmin(fmax(x, 0), 1)).  It is recomputed whenever the volume or the convention changes.

Box test (`intersect`): the reference's test of the unit cube (shaders_common.h:156-184, its __frcp_rn restated as an IEEE
divide) with the literal 0 replaced by lo_k and 1 by hi_k, operation for operation, in float32:

    s_k  = |d_k| < FLT_MIN                                  the reference's quirk: such a slab is IGNORED
    r_k  = 1 / d_k
    l_k  = s_k ? FLT_MAX  : (lo_k - o_k) * r_k
    h_k  = s_k ? -FLT_MAX : (hi_k - o_k) * r_k
    t0   = fmax(t0, fmax(fmax(fmin(l_x, h_x), fmin(l_y, h_y)), fmin(l_z, h_z)))
    t1   = fmin(t1, fmin(fmin(fmax(l_x, h_x), fmax(l_y, h_y)), fmax(l_z, h_z)))
    hit  = t1 > t0  and not empty,      empty = lo_k >= hi_k on any axis

With lo = 0, hi = 1 these are the bits the unclipped kernels compute.  fmin / fmax are IEEE minimumNumber / maximumNumber:
a NaN operand loses, and -0 < +0 (what v_min_f32 / v_max_f32 do; C leaves fmax(+0, -0) to the implementation - it only ever decides
the sign of a zero t0 or t1, for a ray that starts exactly on a face plane).  An empty box is missed by EVERY ray - also by one whose
slab on the empty axis is ignored: the frame is zero and no sample is taken.

The test cuts the primary ray, every shadow ray (what is cut away casts no shadow) and the schedule's block test.  It does not
touch what a tap reads: trilinear taps and gradient taps read the true voxels, also across a clip face, and the gradient's
forward difference flips to a backward one only at the volume's own upper faces.

`ignored_slab_outside`: a ray that hits through an ignored slab with its origin outside that slab's [lo_k, hi_k] - the only
rays that can hit from outside the box's silhouette (the host maps such a frame whole)."""
import numpy as np

from .lighting import fma

F = np.float32
FLT_MIN = F(1.17549435e-38)
FLT_MAX = F(3.4028234663852886e38)


def fmin(a, b):
    """IEEE minimumNumber of float32 arrays: NaN loses, -0 < +0"""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(b) | (a < b), a, b)
        both_zero = (a == 0) & (b == 0)
        return np.where(both_zero, np.where(np.signbit(a), a, b), np.where(np.isnan(a), b, r)).astype(F)


def fmax(a, b):
    """IEEE maximumNumber of float32 arrays: NaN loses, -0 < +0"""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(b) | (a > b), a, b)
        both_zero = (a == 0) & (b == 0)
        return np.where(both_zero, np.where(np.signbit(a), b, a), np.where(np.isnan(a), b, r)).astype(F)


def clamp01(x):
    return fmin(fmax(x, F(0)), F(1))


def volume_constants(dims, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False):
    """(inv_scale, wto_p) of a volume of dims = (nx, ny, nz) voxels, as the host forms them in float32"""
    n = np.asarray(dims, np.int64)
    ext = (n - 1 if vertex_centred else n).astype(F)
    sc = (np.asarray(spacing, F) * ext).astype(F)
    with np.errstate(divide="ignore"):
        inv = (F(1) / sc).astype(F)
    wp = (-(inv * np.asarray(origin, F)).astype(F)).astype(F)
    return inv, wp


def to_object(p, inv_scale, wto_p):
    return fma(np.asarray(p, F), np.asarray(inv_scale, F), np.asarray(wto_p, F))


def object_box(lower, upper, inv_scale, wto_p):
    """the world box -> (lo, hi), the object-space bounds the kernels test"""
    with np.errstate(invalid="ignore"):
        return clamp01(to_object(lower, inv_scale, wto_p)), clamp01(to_object(upper, inv_scale, wto_p))


def is_empty(lo, hi):
    return bool(np.any(np.asarray(lo, F) >= np.asarray(hi, F)))


def intersect(o, d, lo=(0, 0, 0), hi=(1, 1, 1), t0=0.0, t1=FLT_MAX):
    """object-space rays o (n, 3), d (n, 3) against the box [lo, hi] -> (t0 (n,), t1 (n,), hit (n,))"""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.abs(d) < FLT_MIN
        r = (F(1) / d).astype(F)
        l = np.where(s, FLT_MAX, ((lo - o).astype(F) * r).astype(F)).astype(F)
        h = np.where(s, -FLT_MAX, ((hi - o).astype(F) * r).astype(F)).astype(F)
        near, far = fmin(l, h), fmax(l, h)
        a = fmax(np.full(len(o), t0, F), fmax(fmax(near[:, 0], near[:, 1]), near[:, 2]))
        b = fmin(np.full(len(o), t1, F), fmin(fmin(far[:, 0], far[:, 1]), far[:, 2]))
        hit = (b > a) & (not is_empty(lo, hi))
    return a, b, hit


def ignored_slab_outside(o, d, lo=(0, 0, 0), hi=(1, 1, 1)):
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(invalid="ignore"):
        return np.any((np.abs(d) < FLT_MIN) & ~((o >= lo) & (o <= hi)), axis=1)


def world_intervals(org, direction, inv_scale, wto_p, lo=(0, 0, 0), hi=(1, 1, 1)):
    """world-space rays as the march forms their object-space ray (to_object of the origin, the direction scaled by inv_scale
    and NOT renormalised, so t is shared between the two spaces) -> intersect(...): what ovr_hip_clip_intervals returns"""
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        oo = to_object(org, inv_scale, wto_p)
        od = (direction * np.asarray(inv_scale, F)).astype(F)
    return intersect(oo, od, lo, hi)
