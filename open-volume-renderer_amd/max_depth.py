"""The depth limit of the HIP backend (include/ovr_hip.h, ovr_hip_set_max_depth) as a numpy model: the normative text.

Every frame kind fills the whole pixel with volume.  A depth-limited frame ends every ray of a pixel on a ray parameter the caller hands in - the distance of
the opaque surface its own renderer drew there - so that the frame is what lies IN FRONT of that surface and can be blended over the caller's picture
(blend_over).  The ray, the box test and to_object are clipping.py's and camera.py's, the tap and the classification projection.py's, the opacity correction
slice_context.py's, the forward difference and the normal isosurface.normals', the shade factor lighting.shade, the camera normal gradient_opacity.py's:
imported here, not restated.

The image: float32, width * height values in the frame's own pixel order - the order of mapframe's rgba: the value of pixel (ix, iy) at ix + iy * width.
The unit of a value is the march's own t: WORLD LENGTH ALONG THE NORMALISED RAY DIRECTION FROM THE RAY'S ORIGIN.  Under the perspective camera that is the
Euclidean distance from the camera position - not a planar z, not a z-buffer value (ray_distance_from_planar converts an eye-space z).  Under the orthographic
camera it is the distance from the image plane through `from`, the planar depth.

Per pixel sample of pixel (ix, iy) (world origin o, direction d; t0, t1, hit, step = 1 / rate and base = 1 as in the march; float32, fma fused, everything
else rounds on its own):

    z       = depth[ix + iy * width]              every sample of a pixel (spp > 1, jitter) takes the pixel's value
    limited = z < +inf                            false for +inf and for NaN: no surface at this pixel
    tc      = fmin(t1, z) if limited else t1

and from there the march's loop with tc in t1's place, operation for operation - slice_context.py's step 3 with scale 1 under shading NONE, the
gradient-shaded step of gradient_opacity.py with the opacity left unweighted under shading GRADIENT:

    alpha = 0, C = 0, tx = t0, ty = fmin(tc, t0 + step)
    while ty > tx and alpha < 0.9999:             a step of length 0 is not taken; z <= t0 (any negative value, -inf) takes none
        tm = 0.5 * (tx + ty); s = the tap at to_object(fma(tm, d, o)); rgb, a_tf = the classification of s
        a  = opacity_correction(a_tf, base * (ty - tx))              the last step ends on tc and its dt goes through the correction
        under GRADIENT, where a > 0: n_w, n_c and shade from the forward difference at the sample, rgb = clamp01(rgb * shade)
        tr = 1 - alpha; C = fma(tr * clamp01(rgb), a, C); layer = fma(tr * clamp01(n_c), a, layer); alpha = fma(tr, a, alpha)
        tx = ty, ty = fmin(tx + step, tc)

Nothing is composited behind the cut: the pixel is the march's un-premultiplied (rgb, alpha) of what lies in front of the surface.  The gradient layer is
zero under NONE and the march's under GRADIENT.  Counters: samples = steps taken, shaded_samples = steps with a > 0; nothing is skipped, no shadow ray.

Consequences: with z = +inf, NaN or any z >= t1 the sample is the march's bit for bit; with z = the clipped t1 of a clip box that removes only the far side
the frame is the clipped march's; z <= t0 gives zeros and no sample; z = t0 + k * step on a ray whose steps are exact takes exactly k steps."""
import numpy as np

from . import clipping, gradient_opacity, isosurface, lighting, projection
from .clipping import clamp01, fmin
from .gradient_opacity import camera_normal, normal_matrix
from .lighting import fma
from .slice_context import opacity_correction

F = np.float32
NONE, GRADIENT = 0, 1  # the shading modes a depth-limited frame is drawn under
ERT = F(0.9999)        # the march's early-termination literal
BASE = F(1)            # the march's `base`


def check(depth, width, height):
    """the image as ovr_hip_set_max_depth stores it: (height, width) float32; ValueError where it returns EINVAL"""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("the depth image's width and height are at least 1")
    if width > 2 ** 31 - 1 or height > 2 ** 31 - 1 or width * height > 2 ** 31 - 1:
        raise ValueError("the depth image's width x height exceeds 2^31 - 1 pixels")
    d = np.ascontiguousarray(depth, F)
    if d.size != width * height:
        raise ValueError("the depth image holds width * height values")
    return d.reshape(height, width)


def active(on, size=None, fbsize=None, shading=0, slices=0, isovalues=0, projection_mode=0, preintegration=0, gradient_opacity_mode=0):
    """a frame is a depth-limited frame iff the committed frame is the march, the mode is on, the committed shading is NONE or GRADIENT, neither pre-integration
    nor gradient opacity is active (their own rules decide) and the image's size (width, height) equals the committed framebuffer size"""
    march = not slices and not isovalues and not projection_mode
    preintegrated = march and shading == 0 and preintegration == 1
    gradop = gradient_opacity.active(gradient_opacity_mode, shading, slices, isovalues, projection_mode, preintegration)
    same = size is not None and fbsize is not None and tuple(int(v) for v in size) == tuple(int(v) for v in fbsize)
    return bool(on) and march and shading in (NONE, GRADIENT) and not preintegrated and not gradop and same


def cut(t1, z):
    """tc (n,) of the box exits t1 and the pixel values z: fmin(t1, z) where z < +inf, t1 for +inf and NaN"""
    t1, z = np.asarray(t1, F), np.asarray(z, F)
    with np.errstate(invalid="ignore"):
        limited = z < F(np.inf)
        return np.where(limited, fmin(t1, np.where(limited, z, F(0)).astype(F)), t1).astype(F)


def ray_distance_from_planar(basis, size, z, camera_kind=0):
    """the depth image (H, W) float32 of an eye-space planar depth z (H, W) - the distance along the viewing direction from the camera, positive in front of
    it, in the frame's pixel order: under the perspective camera z / cos(angle between the pixel-centre ray and the viewing direction), the Euclidean distance
    from the camera position along the pixel's ray; under the orthographic camera z itself.  Non-finite z stay what they are (+inf: no surface).
    float64 inside, rounded once"""
    w, h = size
    z = np.asarray(z, np.float64).reshape(h, w)
    if camera_kind:
        return z.astype(F)
    d = projection.pixel_rays(basis, w, h, None).reshape(h, w, 3).astype(np.float64)
    axis = np.asarray(basis[1], np.float64)
    axis = axis / np.linalg.norm(axis)
    cos = (d * axis[None, None, :]).sum(-1) / np.linalg.norm(d, axis=-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (z / cos).astype(F)


def blend_over(rgba, rgb):
    """the frame (H, W, 4), un-premultiplied, over the caller's own picture rgb (H, W, 3): rgb_frame * a + own * (1 - a), float32"""
    rgba, rgb = np.asarray(rgba, F), np.asarray(rgb, F)
    a = rgba[..., 3:4]
    return ((rgba[..., :3] * a).astype(F) + (rgb * (F(1) - a).astype(F)).astype(F)).astype(F)


def rays(volume, org, direction, depth, rate, colors, alphas, tf_range, shading=NONE, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL,
         cam_pos=(0, 0, 0), view=None, columns=None, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, camera_kind=0,
         border=1e-5):
    """world rays org, direction (n, 3) - the direction used as given - each ending on depth (n,): dict(steps (taken), tc (the cut; 0 for a ray that is not
    hit), tx (at exit; 0 for a ray that is not hit), shaded (steps with a > 0), rgba (n, 4) and layer (n, 3) of the sample, rays_hit, t0, t1, and - for
    comparisons with a build whose pow differs in its last bits - borderline (a loop test met an alpha within `border` of 0.9999), hinge (the steps from
    t0 to tc of such a ray: what its count may differ by) and borderline_steps (steps whose a > 0 rests on the last bit of the pow: a_tf > 0 and
    a <= 2^-22 with a != a_tf - the shortened last step of a ray may be that short)).  columns: gradient_opacity.normal_matrix of the camera, for the gradient layer under GRADIENT
    (None: the layer stays zero); view: the view vector of every sample under a specular material (the orthographic camera's; None: normalize(cam_pos - pos))"""
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    inv, wp = clipping.volume_constants(dims, spacing, origin, vertex_centred)
    blo, bhi = ((0, 0, 0), (1, 1, 1)) if clip is None else clip
    if camera_kind:
        from . import camera
        t0, t1, hit = camera.hits(org, direction, inv, wp, blo, bhi, camera_kind)
    else:
        t0, t1, hit = clipping.world_intervals(org, direction, inv, wp, blo, bhi)
    m_rays = len(t0)
    z = np.broadcast_to(np.asarray(depth, F).reshape(-1), (m_rays,)) if np.size(depth) in (1, m_rays) else None
    if z is None:
        raise ValueError("one depth per ray")
    tc = cut(t1, z)
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    L = lighting.normalize(np.asarray(lighting.LITERAL_LIGHT if light is None else light, F))
    ka, kd, ks, shin = material
    step = F(1) / F(rate)
    alpha, C, layer = np.zeros(m_rays, F), np.zeros((m_rays, 3), F), np.zeros((m_rays, 3), F)
    steps, shaded, tiny = np.zeros(m_rays, np.int64), np.zeros(m_rays, np.int64), np.zeros(m_rays, np.int64)
    near = np.zeros(m_rays, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tx = t0.copy()
        ty = fmin(tc, (t0 + step).astype(F))
        live = hit.copy()
        while True:
            near |= live & (ty > tx) & (np.abs(alpha.astype(np.float64) - float(ERT)) <= border)
            live = live & (ty > tx) & (alpha < ERT)
            idx = np.flatnonzero(live)
            if not idx.size:
                break
            x, y = tx[idx], ty[idx]
            tm = (F(0.5) * (x + y).astype(F)).astype(F)
            pos = fma(tm[:, None], direction[idx], org[idx])
            po = clipping.to_object(pos, inv, wp)
            s = tap(po)
            c = projection.classify(s, colors, alphas, *tf_range)
            a = opacity_correction(c[:, 3], BASE, (y - x).astype(F))
            rgb = c[:, :3]
            n_c = np.zeros((idx.size, 3), F)
            lit = a > 0
            if shading == GRADIENT and lit.any():
                n_w = isosurface.normals(tap, po[lit], s[lit], dims, inv, vertex_centred)
                f = lighting.shade(n_w, pos[lit], np.zeros(int(lit.sum()), F), L, cam_pos, ka, kd, ks, shin, intensity, view=view)
                rgb = rgb.copy()
                rgb[lit] = (rgb[lit] * f[:, None]).astype(F)
                if columns is not None:
                    n_c[lit] = clamp01(camera_normal(n_w, columns))
            tr = (F(1) - alpha[idx]).astype(F)
            C[idx] = fma((tr[:, None] * clamp01(rgb)).astype(F), a[:, None], C[idx])
            if shading == GRADIENT:
                layer[idx] = fma((tr[:, None] * n_c).astype(F), a[:, None], layer[idx])
            alpha[idx] = fma(tr, a, alpha[idx])
            steps[idx] += 1
            shaded[idx] += lit
            tiny[idx] += (c[:, 3] > 0) & (a <= F(2.0 ** -22)) & (a != c[:, 3])
            tx = np.where(live, ty, tx).astype(F)
            ty = np.where(live, fmin((tx + step).astype(F), tc), ty).astype(F)
    _, whole = projection.steps(t0, tc, step, hit & (tc > t0))
    rgba = np.zeros((m_rays, 4), F)
    posa = alpha > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(posa, alpha, F(1))[:, None]
        rgba[:, :3] = np.where(posa[:, None], (C / den).astype(F), F(0))
        out_layer = np.where(posa[:, None], (layer / den).astype(F), F(0)).astype(F)
    rgba[:, 3] = alpha
    zero = F(0)
    return dict(steps=steps, tc=np.where(hit, tc, zero).astype(F), tx=np.where(hit, tx, zero).astype(F), shaded=shaded, rgba=rgba, layer=out_layer, rays_hit=hit,
                t0=t0, t1=t1, borderline=near, hinge=np.where(near, whole, 0), borderline_steps=tiny)


def frame(volume, basis, size, depth, rate, colors, alphas, tf_range, shading=NONE, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL,
          spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, spp=1, noise=None, frame_index=1, camera_kind=0, columns=None):
    """one depth-limited frame: rgba (H, W, 4), the gradient layer (H, W, 3) and counters (rays, rays_hit, active_pixels, samples, shaded; hinge, borderline_steps and the
    borderline pixel mask, see rays).  depth: the image (H, W) in the frame's pixel order; the other arguments are gradient_opacity.frame's without the ramp"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    z = check(depth, w, h).reshape(-1)
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, rays_hit=0, active_pixels=h * w, samples=0, shaded=0, hinge=0, borderline_steps=0)
    borderline = np.zeros(h * w, bool)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    columns = normal_matrix(basis) if columns is None else columns
    view = None
    for j in range(spp):
        xi = None if noise is None else projection.blue_noise_variates(noise, w, h, frame_index, spp, j)
        d = projection.pixel_rays(basis, w, h, xi).reshape(-1, 3)
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
            view = camera.view_vector(basis) if camera_kind == camera.ORTHOGRAPHIC else None
        r = rays(volume, org, d, z, rate, colors, alphas, tf_range, shading, light, intensity, material, basis[0], view, columns, spacing, origin,
                 vertex_centred, clip, sampler, camera_kind)
        rgba = (rgba + r["rgba"]).astype(F)
        layer = (layer + r["layer"]).astype(F)
        counters["rays"] += h * w
        counters["rays_hit"] += int(r["rays_hit"].sum())
        counters["samples"] += int(r["steps"].sum())
        counters["shaded"] += int(r["shaded"].sum())
        counters["hinge"] += int(r["hinge"].sum())
        counters["borderline_steps"] += int(r["borderline_steps"].sum())
        borderline |= r["borderline"]
    counters["borderline"] = borderline.reshape(h, w)
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
