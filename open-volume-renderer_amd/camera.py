"""The cameras of the HIP backend (include/ovr_hip.h, ovr_hip_set_camera / ovr_hip_set_camera_orthographic) as a numpy model: the normative text.

Everything is float32; every product and sum rounds on its own (the kernels are built with -ffp-contract=off), fma is a fused multiply-add.

The basis (`basis`): the host's expressions (device_impl.cpp:125-144) for both kinds; only the scalar t differs.

    t      = 2 tanf(fovy / 2 * pi / 180)        PERSPECTIVE
    t      = height                             ORTHOGRAPHIC: the world height of the image; height * aspect is its width
    dir    = normalize(at - from)
    aspect = float(W) / float(H)
    hor    = (t * aspect) * normalize(cross(dir, up))
    ver    = cross(hor, dir) / aspect
    pos    = from

The ray of a pixel sample (`pixel_rays`): the screen offsets are formed as projection.pixel_rays forms them,

    sx = (ix + .5) * (1 / W) [+ (xi0 - .5) * (1 / W)],  ux = sx - .5        sy, uy likewise with H; xi: the sample's jitter variates, if any

    PERSPECTIVE   org = pos                                      dir_s = normalize_exact((dir + ux * hor) + uy * ver)
    ORTHOGRAPHIC  org_k = (pos_k + ux * hor_k) + uy * ver_k      dir_s = dir, as stored, not renormalised

- the direction expression's shape with the roles of position and direction swapped.  dir is a unit vector, so the ray parameter t is the world distance
from the image plane through `from`: the depths of the projection and isosurface layers are planar under this camera, and what lies behind the plane is not
seen (t0 >= 0).  The object-space ray is oo = to_object(org) per sample, od = dir_s * inv_scale.

The hit (`hits`): PERSPECTIVE clipping.intersect's - the reference's box test with its quirk, a slab whose direction component is below FLT_MIN is ignored.
ORTHOGRAPHIC: intersect's hit AND NOT clipping.ignored_slab_outside.  Under a perspective camera only the odd ray has such a component; under an
orthographic camera along a volume axis EVERY ray has two, and the quirk would report every ray of the frame as a hit and smear the clamped edge voxels over
the image (32 x 16 x 8 volume, 64 x 32 frame along -z at height 32: 2048 hits, 1536 of them outside the silhouette).  A ray outside an ignored slab misses:
the geometric truth.  A miss is a counted ray with no step and a zero pixel.

The view vector of the specular term (`view_vector`): V = -dir for every sample (lighting.shade's `view=`); the perspective camera's is normalize(pos - p).

`auto_height`: scene files carry a projection mode and no height: height = 2 |eye - center| tan(fovy / 2), the parallel view with the perspective view's
extent at the plane through `center`."""
import math

import numpy as np

from . import clipping
from . import projection

F = np.float32
PERSPECTIVE, ORTHOGRAPHIC = 0, 1


def basis(eye, at, up, width, height, fovy=60.0, orthographic_height=None):
    """(pos, dir, hor, ver); orthographic_height: None = the perspective camera of `fovy` degrees, else the orthographic camera of that world height"""
    if orthographic_height is None:
        return projection.camera_basis(eye, at, up, fovy, width, height)
    eye, at, up = (np.asarray(v, F) for v in (eye, at, up))

    def norm(v):
        l = np.sqrt(projection.fma(v[0], v[0], projection.fma(v[1], v[1], F(v[2] * v[2]))))
        return ((v * F(1)) / l).astype(F)

    def cross(a, b):
        return np.array([F(a[1] * b[2]) - F(b[1] * a[2]), F(a[2] * b[0]) - F(b[2] * a[0]), F(a[0] * b[1]) - F(b[0] * a[1])], F)

    t = F(orthographic_height)
    aspect = F(width) / F(height)
    d = norm((at - eye).astype(F))
    hor = (F(t * aspect) * norm(cross(d, up))).astype(F)
    ver = (cross(hor, d) / aspect).astype(F)
    return eye, d, hor, ver


def screen_offsets(width, height, xi=None):
    """(ux, uy), each (H, W): the sample's screen position minus one half, as the kernels form it"""
    rsx, rsy = F(1) / F(width), F(1) / F(height)
    sx = ((np.arange(width, dtype=F) + F(0.5)) * rsx).astype(F)[None, :].repeat(height, 0)
    sy = ((np.arange(height, dtype=F) + F(0.5)) * rsy).astype(F)[:, None].repeat(width, 1)
    if xi is not None:
        sx = (sx + ((np.asarray(xi[0], F) - F(0.5)).astype(F) * rsx).astype(F)).astype(F)
        sy = (sy + ((np.asarray(xi[1], F) - F(0.5)).astype(F) * rsy).astype(F)).astype(F)
    return (sx - F(0.5)).astype(F), (sy - F(0.5)).astype(F)


def pixel_rays(cam_basis, width, height, xi=None, kind=PERSPECTIVE):
    """(org (H, W, 3), dir (H, W, 3)) of the pixel samples in world space; xi = (xi0, xi1), each (H, W): the jitter variates, None = the pixel centre"""
    pos, d, hor, ver = (np.asarray(v, F) for v in cam_basis)
    if kind == PERSPECTIVE:
        return np.broadcast_to(pos, (height, width, 3)).copy(), projection.pixel_rays(cam_basis, width, height, xi)
    ux, uy = screen_offsets(width, height, xi)
    org = np.empty((height, width, 3), F)
    for k in range(3):
        org[..., k] = ((pos[k] + (ux * hor[k]).astype(F)).astype(F) + (uy * ver[k]).astype(F)).astype(F)
    return org, np.broadcast_to(d, (height, width, 3)).copy()


def hits(org, direction, inv_scale, wto_p, lo=(0, 0, 0), hi=(1, 1, 1), kind=PERSPECTIVE):
    """(t0, t1, hit) of world rays as the primary rays of a frame are tested: the orthographic camera's miss rule on top of clipping.world_intervals"""
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    t0, t1, hit = clipping.world_intervals(org, direction, inv_scale, wto_p, lo, hi)
    if kind == ORTHOGRAPHIC:
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            oo = clipping.to_object(org, inv_scale, wto_p)
            od = (direction * np.asarray(inv_scale, F)).astype(F)
        hit = hit & ~clipping.ignored_slab_outside(oo, od, lo, hi)
    return t0, t1, hit


def view_vector(cam_basis):
    """the orthographic camera's view vector: -dir, as stored"""
    return (-np.asarray(cam_basis[1], F)).astype(F)


def auto_height(eye, center, fovy):
    """the orthographic height that shows what the perspective camera of `fovy` degrees shows at the plane through `center` (scene files carry no height)"""
    d = math.sqrt(sum((float(a) - float(b)) ** 2 for a, b in zip(eye, center)))
    return 2.0 * d * math.tan(math.radians(float(fovy)) * 0.5)
