"""The depth layer of the HIP backend (include/ovr_hip.h, ovr_hip_set_depth_output) as a numpy model: the normative text.

A march frame is (rgb, alpha).  A depth frame is the same picture, bit for bit, and in the framebuffer's second layer - the buffer mapframe hands out as
`grad` - WHERE along each ray that picture is: the counterpart of the depth limit (max_depth.py).  The ray, the box test, the cut, the tap, the
classification, the opacity correction and the gradient-shaded step are max_depth.py's own pieces, imported here and not restated; the loop below is
max_depth.rays' loop with four more values.

Per pixel sample (t0, t1, hit, step, tc exactly as max_depth.py forms them: tc = t1 where no limit applies, the cut where one does), float32, fma fused:

    alpha = 0, C = 0, S = 0, d = 0, reached = False, k = 0, n = 0, tx = t0, ty = fmin(tc, t0 + step)
    while ty > tx and alpha < 0.9999:
        tm, a, rgb as in max_depth.py
        tr = 1 - alpha; C = fma(tr * clamp01(rgb), a, C); S = fma(tr * tm, a, S); alpha = fma(tr, a, alpha); n += 1
        if not reached and a > 0 and alpha >= tau: reached, d, k = True, ty, n          ty: the BACK end of the crossing step
        tx = ty, ty = fmin(tx + step, tc)

The sample's layer is (d if reached else 0, S, 1 if reached else 0).  Samples per pixel sum and are scaled by 1 / spp; like the march's gradient layer the
layer of an accumulated frame is the LAST frame's (write_pixel accumulates rgba alone).  resolve() turns a frame into depths.

Units: every depth is the march's own t - what ovr_hip_set_max_depth takes; planar_from_ray_distance inverts max_depth.ray_distance_from_planar.
tau lies in (0, 0.9999]: TAU_FIRST, the smallest positive normal float, gives the back end of the first step with opacity, 0.5 the "median" surface; above
the early-termination literal a crossing could only happen by overshoot.  ty is recorded and not tm: handed back as a depth limit, fmin(tx + step, d) == d
on the crossing step, and the limited march takes exactly the same k steps with the same bits."""
import numpy as np

from . import clipping, isosurface, lighting, max_depth, projection
from .clipping import clamp01, fmin
from .lighting import fma
from .max_depth import BASE, ERT, GRADIENT, NONE, cut
from .slice_context import opacity_correction

F = np.float32
OFF, ON = 0, 1
TAU_FIRST = float(np.finfo(F).tiny)   # the smallest positive normal float: any step with opacity crosses it
TAU_MAX = float(ERT)                  # 0.9999f


def check(mode, threshold=0.0):
    """(mode, threshold as float32) as ovr_hip_set_depth_output stores them; ValueError where it returns EINVAL"""
    if mode not in (OFF, ON):
        raise ValueError("the depth output's mode is OFF or ON")
    if mode == OFF:
        return OFF, F(0)
    t = F(threshold)
    if not (t > F(0)) or not (t <= ERT):
        raise ValueError("the depth output's threshold lies in (0, 0.9999]")
    return ON, t


def active(mode, shading=0, slices=0, isovalues=0, projection_mode=0, preintegration=0, gradient_opacity_mode=0):
    """a frame is a depth frame iff the committed frame is the march, the mode is ON, the committed shading is NONE or GRADIENT, and neither pre-integration nor
    gradient opacity is active (their own rules decide) - max_depth.active without the image's size"""
    return max_depth.active(mode == ON, (1, 1), (1, 1), shading, slices, isovalues, projection_mode, preintegration, gradient_opacity_mode)


def limited(mode, max_depth_on, size=None, fbsize=None, **state):
    """a depth frame applies the committed depth image iff the depth limit's own rule draws it"""
    return active(mode, **state) and max_depth.active(max_depth_on, size, fbsize, **state)


def planar_from_ray_distance(basis, size, t, camera_kind=0):
    """the inverse of max_depth.ray_distance_from_planar: the eye-space planar depth (H, W) float32 of a ray-distance image t (H, W): under the perspective
    camera t * cos(angle between the pixel-centre ray and the viewing direction), under the orthographic camera t itself.  Non-finite t stay what they are.
    float64 inside, rounded once"""
    w, h = size
    t = np.asarray(t, np.float64).reshape(h, w)
    if camera_kind:
        return t.astype(F)
    d = projection.pixel_rays(basis, w, h, None).reshape(h, w, 3).astype(np.float64)
    axis = np.asarray(basis[1], np.float64)
    axis = axis / np.linalg.norm(axis)
    cos = (d * axis[None, None, :]).sum(-1) / np.linalg.norm(d, axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return (t * cos).astype(F)


def resolve(rgba, layer):
    """(threshold depth, alpha-weighted mean depth, share) of a finished frame, each the frame's shape without the channel axis, float32: layer[0] / layer[2]
    where layer[2] > 0, layer[1] / rgba[3] where rgba[3] > 0, layer[2]; +inf - the depth limit's "no surface" - where a depth is undefined"""
    rgba, layer = np.asarray(rgba, F), np.asarray(layer, F)
    share, a = layer[..., 2], rgba[..., 3]
    inf = F(np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = np.where(share > 0, (layer[..., 0] / np.where(share > 0, share, F(1))).astype(F), inf).astype(F)
        mean = np.where(a > 0, (layer[..., 1] / np.where(a > 0, a, F(1))).astype(F), inf).astype(F)
    return thr, mean, share.astype(F)


def rays(volume, org, direction, tau, rate, colors, alphas, tf_range, depth=None, shading=NONE, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL,
         cam_pos=(0, 0, 0), view=None, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, camera_kind=0, border=1e-5):
    """max_depth.rays with the depth accumulators (depth None: no limit on any ray): its dict - steps, tc, tx, shaded, rgba, rays_hit, t0, t1, borderline, hinge,
    borderline_steps - and reached (n,) bool, d (n,) float32, k (n,) int64, S (n,) float32, layer (n, 3) = (d, S, reached), and near_tau: a crossing test met
    an alpha within border * tau of tau (with the termination's `borderline`, what a build whose pow differs in its last bits may decide differently);
    tiny_before: steps counted in borderline_steps that were taken before the crossing (at the smallest tau such a step IS the crossing or not)"""
    _, tau = check(ON, tau)
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
    if depth is None:
        tc = t1.copy()
    else:
        if np.size(depth) not in (1, m_rays):
            raise ValueError("one depth per ray")
        tc = cut(t1, np.broadcast_to(np.asarray(depth, F).reshape(-1), (m_rays,)))
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    L = lighting.normalize(np.asarray(lighting.LITERAL_LIGHT if light is None else light, F))
    ka, kd, ks, shin = material
    step = F(1) / F(rate)
    alpha, C = np.zeros(m_rays, F), np.zeros((m_rays, 3), F)
    S, d = np.zeros(m_rays, F), np.zeros(m_rays, F)
    reached, k = np.zeros(m_rays, bool), np.zeros(m_rays, np.int64)
    steps, shaded, tiny, tiny_before = np.zeros(m_rays, np.int64), np.zeros(m_rays, np.int64), np.zeros(m_rays, np.int64), np.zeros(m_rays, np.int64)
    near, near_tau = np.zeros(m_rays, bool), np.zeros(m_rays, bool)
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
            lit = a > 0
            if shading == GRADIENT and lit.any():
                n_w = isosurface.normals(tap, po[lit], s[lit], dims, inv, vertex_centred)
                f = lighting.shade(n_w, pos[lit], np.zeros(int(lit.sum()), F), L, cam_pos, ka, kd, ks, shin, intensity, view=view)
                rgb = rgb.copy()
                rgb[lit] = (rgb[lit] * f[:, None]).astype(F)
            tr = (F(1) - alpha[idx]).astype(F)
            C[idx] = fma((tr[:, None] * clamp01(rgb)).astype(F), a[:, None], C[idx])
            S[idx] = fma((tr * tm).astype(F), a, S[idx])
            alpha[idx] = fma(tr, a, alpha[idx])
            steps[idx] += 1
            shaded[idx] += lit
            is_tiny = (c[:, 3] > 0) & (a <= F(2.0 ** -22)) & (a != c[:, 3])
            tiny[idx] += is_tiny
            tiny_before[idx] += is_tiny & ~reached[idx]
            fresh = ~reached[idx]
            near_tau[idx] |= fresh & lit & (np.abs(alpha[idx].astype(np.float64) - float(tau)) <= border * float(tau))
            crossing = fresh & lit & (alpha[idx] >= tau)
            at = idx[crossing]
            reached[at] = True
            d[at] = y[crossing]
            k[at] = steps[at]
            tx = np.where(live, ty, tx).astype(F)
            ty = np.where(live, fmin((tx + step).astype(F), tc), ty).astype(F)
    _, whole = projection.steps(t0, tc, step, hit & (tc > t0))
    rgba = np.zeros((m_rays, 4), F)
    posa = alpha > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(posa, alpha, F(1))[:, None]
        rgba[:, :3] = np.where(posa[:, None], (C / den).astype(F), F(0))
    rgba[:, 3] = alpha
    zero = F(0)
    layer = np.stack([d, S, reached.astype(F)], axis=1).astype(F)
    return dict(steps=steps, tc=np.where(hit, tc, zero).astype(F), tx=np.where(hit, tx, zero).astype(F), shaded=shaded, rgba=rgba, layer=layer, rays_hit=hit, t0=t0, t1=t1,
                borderline=near, hinge=np.where(near, whole, 0), borderline_steps=tiny, reached=reached, d=d, k=k, S=S, near_tau=near_tau, tiny_before=tiny_before)


def borderline_rays(r, tau):
    """the rays of rays()' dict that a build whose pow differs in its last bits may decide differently: a loop test within `border` of 0.9999, a crossing test
    within border * tau of tau, and - at the smallest tau, where any a > 0 crosses - a ray with a step before its crossing whose a > 0 rests on the pow's last bit"""
    b = r["borderline"] | r["near_tau"]
    if F(tau) == F(TAU_FIRST):
        b = b | (r["tiny_before"] > 0)
    return b


def frame(volume, basis, size, tau, rate, colors, alphas, tf_range, depth=None, shading=NONE, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL,
          spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, spp=1, noise=None, frame_index=1, camera_kind=0):
    """one depth frame: rgba (H, W, 4), the layer (H, W, 3) and max_depth.frame's counters (borderline: the pixel mask of borderline_rays over the samples).
    depth: the committed image (H, W) in the frame's pixel order, or None; the other arguments are max_depth.frame's"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    z = None if depth is None else max_depth.check(depth, w, h).reshape(-1)
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, rays_hit=0, active_pixels=h * w, samples=0, shaded=0, hinge=0, borderline_steps=0)
    borderline = np.zeros(h * w, bool)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    view = None
    for j in range(spp):
        xi = None if noise is None else projection.blue_noise_variates(noise, w, h, frame_index, spp, j)
        dirs = projection.pixel_rays(basis, w, h, xi).reshape(-1, 3)
        if camera_kind:
            from . import camera
            org, dirs = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
            view = camera.view_vector(basis) if camera_kind == camera.ORTHOGRAPHIC else None
        r = rays(volume, org, dirs, tau, rate, colors, alphas, tf_range, z, shading, light, intensity, material, basis[0], view, spacing, origin, vertex_centred,
                 clip, sampler, camera_kind)
        rgba = (rgba + r["rgba"]).astype(F)
        layer = (layer + r["layer"]).astype(F)
        counters["rays"] += h * w
        counters["rays_hit"] += int(r["rays_hit"].sum())
        counters["samples"] += int(r["steps"].sum())
        counters["shaded"] += int(r["shaded"].sum())
        counters["hinge"] += int(r["hinge"].sum())
        counters["borderline_steps"] += int(r["borderline_steps"].sum())
        borderline |= borderline_rays(r, tau)
    counters["borderline"] = borderline.reshape(h, w)
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
