"""Gradient opacity of the HIP backend (include/ovr_hip.h, ovr_hip_set_gradient_opacity) as a numpy model: the normative text.

The march classifies a sample by its value alone: one tap, one lookup in the 1-D transfer function.  A gradient-opacity frame weights the table's opacity of
every sample by a ramp over the magnitude of the local gradient (Levoy 1988; VTK's "gradient opacity"): the inside of a homogeneous material fades, its
boundaries stay.  The ray, the box test and to_object are clipping.py's and camera.py's, the tap and the classification projection.py's, the opacity correction
slice_context.py's, the normal isosurface.normals', the shade factor lighting.shade: imported here, not restated.

State (commit): (mode, lo, hi) with lo < hi, both finite, lo may be negative; in mode OFF the thresholds are ignored and stored as (0, 1).
inv_ramp = 1 / (hi - lo), once, in float32.

Per pixel sample (world origin o, direction d; t0, t1, hit, step = 1 / rate and base = 1 as in the unshaded march; float32, fma fused, everything else rounds on
its own) the loop is slice_context.py's step 3 with tc = t1 and scale 1.  After the tap s at po and a_tf, rgb from the march's classification:

    if a_tf > 0:                                  otherwise no gradient is fetched: a_tf * w is 0 whatever w
        d_k = -g_k if po_k + g_k > 1 else g_k     g_k = 1 / n_k (vertex-centred: 1 / (n_k - 1)): the shading's forward difference
        G_k = (tap(po + d_k e_k) - s) / d_k
        W_k = G_k * inv_scale_k                   the world gradient, sample units per world length
        m   = sqrt(fma(Wx, Wx, fma(Wy, Wy, Wz * Wz))) * tf_scale      tf_scale: tf_coord's scale, 0 for a degenerate range
        w   = clamp01((m - lo) * inv_ramp)
        a_tf = a_tf * w
    a = opacity_correction(a_tf, base * (ty - tx))

m is "fraction of the transfer function's range per world unit length" and does not depend on the voxel type.  Under shading NONE the composite is the march's and
the gradient layer zero.  Under shading GRADIENT a step with a > 0 uses the same G for the light: n_w = isosurface.normals' normal, n_c = normalize(the camera's
normal matrix applied to n_w), shade = lighting.shade(n_w, ..., shadow 0), C = fma(tr * clamp01(rgb * shade), a, C), and the gradient layer accumulates
fma(tr * clamp01(n_c), a, .) - operation for operation the GRADIENT-shaded march.

Counters: samples = steps taken; shaded_samples = steps with a > 0; nothing is skipped.  The number of steps that fetched a gradient is reported per ray.

Consequences (x * 1 and x * 0.5 are exact): with (lo, hi) = (-1, 0) w == 1 for every m >= 0 and the frame is the same state's OFF frame bit for bit; over a
constant volume with lo >= 0 every w is 0 and the frame is zero; where every m is exactly 1/16 and the ramp is (0, 1/8) every w is exactly 0.5 and the rays are
the march's under the alpha table times 0.5; with hi at half a ramp's slope w == 1 whatever the rounding of m."""
import numpy as np

from . import clipping, isosurface, lighting, projection
from .clipping import clamp01, fmin
from .lighting import fma
from .slice_context import opacity_correction

F = np.float32
OFF, RAMP = 0, 1
NONE, GRADIENT = 0, 1  # the shading modes a gradient-opacity frame is drawn under
ERT = F(0.9999)        # the march's early-termination literal
BASE = F(1)            # the march's `base`


def commit(mode, lo=0.0, hi=1.0):
    """(mode, lo, hi, inv_ramp) as ovr_hip_set_gradient_opacity stores them (float32); ValueError where it returns EINVAL.  In mode OFF the thresholds are ignored,
    but for being finite, and stored as (0, 1)"""
    if mode not in (OFF, RAMP):
        raise ValueError("the gradient-opacity mode is OFF or RAMP")
    with np.errstate(over="ignore", invalid="ignore"):
        lo, hi = F(lo), F(hi)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("the gradient-opacity thresholds are finite")
        if int(mode) == OFF:
            return OFF, F(0), F(1), F(1)
        width = F(hi - lo)
        if not (lo < hi) or not np.isfinite(width) or not width > 0:
            raise ValueError("the gradient-opacity thresholds satisfy lo < hi")
        return RAMP, lo, hi, F(F(1) / width)


def active(mode, shading=0, slices=0, isovalues=0, projection_mode=0, preintegration=0):
    """a frame is a gradient-opacity frame iff the committed frame is the march, the mode is RAMP, the committed shading is NONE or GRADIENT and the frame is not
    a pre-integrated one (preintegration: its committed mode; its own rule - the march under shading NONE - decides whether it is drawn)"""
    march = not slices and not isovalues and not projection_mode
    preintegrated = march and shading == 0 and preintegration == 1
    return int(mode) == RAMP and march and shading in (NONE, GRADIENT) and not preintegrated


def tf_scale(tf_range):
    lower, upper = F(tf_range[0]), F(tf_range[1])
    return F(0) if upper == lower else F(F(1) / F(upper - lower))


def difference(tap_object, po, s, dims, vertex_centred=False):
    """the forward difference G (n, 3) at the object positions po (n, 3) with the samples s there: one-sided, flipped at the upper bound"""
    n = np.asarray(dims, np.int64)
    g = (F(1) / (n - 1 if vertex_centred else n).astype(F)).astype(F)
    grad = np.empty(po.shape, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(3):
            d = np.where((po[:, k] + g[k]).astype(F) > F(1), -g[k], g[k]).astype(F)
            pk = po.copy()
            pk[:, k] = (po[:, k] + d).astype(F)
            grad[:, k] = ((tap_object(pk) - s).astype(F) / d).astype(F)
    return grad


def magnitude(grad, inv_scale, scale):
    """m (n,) of the object-space differences grad (n, 3): the world gradient's length times the transfer function's scale"""
    with np.errstate(invalid="ignore", over="ignore"):
        w = (np.asarray(grad, F) * np.asarray(inv_scale, F)[None, :]).astype(F)
        return (np.sqrt(lighting.dot(w, w)).astype(F) * F(scale)).astype(F)


def weight(m, lo, inv_ramp):
    with np.errstate(invalid="ignore", over="ignore"):
        return clamp01(((np.asarray(m, F) - F(lo)).astype(F) * F(inv_ramp)).astype(F))


def magnitudes(volume, tf_range, spacing=(1, 1, 1), vertex_centred=False):
    """the model's m at the voxel centres (nz, ny, nx), so that thresholds can be chosen from percentiles.  tf_range in the samples' units
    (projection.normalized_range)"""
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    inv, _ = clipping.volume_constants(dims, spacing, (0, 0, 0), vertex_centred)
    ext = [n - 1 if vertex_centred else n for n in dims]
    axes = [((np.arange(n, dtype=F) + (F(0) if vertex_centred else F(0.5))) / F(e)).astype(F) for n, e in zip(dims, ext)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    po = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(F)
    tap = lambda p: projection.sample(vol, p, vertex_centred)
    return magnitude(difference(tap, po, tap(po), dims, vertex_centred), inv, tf_scale(tf_range)).reshape(nz, ny, nx)


def normal_matrix(basis):
    """the inverse transpose of the camera's world-to-camera rotation, as the march forms it for the gradient layer: columns (3, 3), c_j = cross / det"""
    _, d, hor, ver = (np.asarray(v, F) for v in basis)
    x, y = lighting.normalize(hor), lighting.normalize(ver)
    z = (-lighting.normalize(d)).astype(F)
    vx, vy, vz = (np.array([x[k], y[k], z[k]], F) for k in range(3))
    cross = lambda a, b: np.array([F(a[1] * b[2]) - F(b[1] * a[2]), F(a[2] * b[0]) - F(b[2] * a[0]), F(a[0] * b[1]) - F(b[0] * a[1])], F)
    det = lighting.dot(vx, cross(vy, vz))
    return np.stack([(cross(vy, vz) / det).astype(F), (cross(vz, vx) / det).astype(F), (cross(vx, vy) / det).astype(F)], 0)


def camera_normal(n_w, columns):
    """normalize(n_w.x * c0 + n_w.y * c1 + n_w.z * c2), the sums as fmas from the right"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.stack([fma(n_w[:, 0], columns[0][k], fma(n_w[:, 1], columns[1][k], (n_w[:, 2] * columns[2][k]).astype(F))) for k in range(3)], 1)
        return lighting.normalize(v)


def rays(volume, org, direction, rate, colors, alphas, tf_range, lo, hi, shading=NONE, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL,
         cam_pos=(0, 0, 0), view=None, columns=None, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, camera_kind=0,
         border=1e-5, w_border=1e-4):
    """world rays org, direction (n, 3) - the direction used as given - under the ramp (lo, hi): dict(steps (taken), gradients (of them steps that fetched a
    gradient), tx (at exit; 0 for a ray that is not hit), shaded (steps with a > 0), rgba (n, 4) and layer (n, 3) of the sample, rays_hit, w_min / w_max (the
    extreme weights of the ray's gradient steps; 1 / 0 without one), and - for comparisons with a build whose pow or gradient differ in their last bits -
    borderline (a loop test met an alpha within `border` of 0.9999), hinge (the steps from t0 to t1 of such a ray: what its count may differ by), w_borderline
    (gradient steps whose (m - lo) * inv_ramp lies within w_border of 0: whether a > 0 rests on the last bits of m)).
    columns: normal_matrix of the camera, for the gradient layer under GRADIENT (None: the layer stays zero); view: the view vector of every sample under a
    specular material (the orthographic camera's; None: normalize(cam_pos - pos))"""
    _, lo, hi, inv_ramp = commit(RAMP, lo, hi)
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
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    scale = tf_scale(tf_range)
    L = lighting.normalize(np.asarray(lighting.LITERAL_LIGHT if light is None else light, F))
    ka, kd, ks, shin = material
    step = F(1) / F(rate)
    alpha, C, layer = np.zeros(m_rays, F), np.zeros((m_rays, 3), F), np.zeros((m_rays, 3), F)
    steps, gradients, shaded, w_near = (np.zeros(m_rays, np.int64) for _ in range(4))
    w_min, w_max = np.ones(m_rays, F), np.zeros(m_rays, F)
    near = np.zeros(m_rays, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tx = t0.copy()
        ty = fmin(t1, (t0 + step).astype(F))
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
            a_tf = c[:, 3].copy()
            need = a_tf > 0
            G = np.zeros((idx.size, 3), F)
            if need.any():
                G[need] = difference(tap, po[need], s[need], dims, vertex_centred)
                mm = magnitude(G[need], inv, scale)
                w = weight(mm, lo, inv_ramp)
                a_tf[need] = (a_tf[need] * w).astype(F)
                ridx = idx[need]
                np.minimum.at(w_min, ridx, w)
                np.maximum.at(w_max, ridx, w)
                np.add.at(w_near, ridx, np.abs((mm.astype(np.float64) - float(lo)) * float(inv_ramp)) <= w_border)
            a = opacity_correction(a_tf, BASE, (y - x).astype(F))
            rgb = c[:, :3]
            n_c = np.zeros((idx.size, 3), F)
            lit = a > 0
            if shading == GRADIENT and lit.any():
                n_w = isosurface.normals(tap, po[lit], s[lit], dims, inv, vertex_centred)
                v = None if view is None else view
                f = lighting.shade(n_w, pos[lit], np.zeros(int(lit.sum()), F), L, cam_pos, ka, kd, ks, shin, intensity, view=v)
                rgb = rgb.copy()
                rgb[lit] = clamp01((rgb[lit] * f[:, None]).astype(F))
                if columns is not None:
                    n_c[lit] = clamp01(camera_normal(n_w, columns))
            tr = (F(1) - alpha[idx]).astype(F)
            C[idx] = fma((tr[:, None] * rgb).astype(F), a[:, None], C[idx])
            if shading == GRADIENT:
                layer[idx] = fma((tr[:, None] * n_c).astype(F), a[:, None], layer[idx])
            alpha[idx] = fma(tr, a, alpha[idx])
            steps[idx] += 1
            gradients[idx] += need
            shaded[idx] += lit
            tx = np.where(live, ty, tx).astype(F)
            ty = np.where(live, fmin((tx + step).astype(F), t1), ty).astype(F)
    _, whole = projection.steps(t0, t1, step, hit)
    rgba = np.zeros((m_rays, 4), F)
    posa = alpha > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(posa, alpha, F(1))[:, None]
        rgba[:, :3] = np.where(posa[:, None], (C / den).astype(F), F(0))
        out_layer = np.where(posa[:, None], (layer / den).astype(F), F(0)).astype(F)
    rgba[:, 3] = alpha
    return dict(steps=steps, gradients=gradients, tx=np.where(hit, tx, F(0)).astype(F), shaded=shaded, rgba=rgba, layer=out_layer, rays_hit=hit, w_min=w_min,
                w_max=w_max, borderline=near, hinge=np.where(near, whole, 0), w_borderline=w_near)


def frame(volume, basis, size, rate, colors, alphas, tf_range, lo, hi, shading=NONE, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL,
          spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, spp=1, noise=None, frame_index=1, camera_kind=0, columns=None):
    """one gradient-opacity frame: rgba (H, W, 4), the gradient layer (H, W, 3) and counters (rays, active_pixels, samples, shaded, gradients; hinge, w_borderline
    and the borderline pixel mask, see rays).  The arguments are preintegration.frame's with the ramp, the shading mode, light and material; columns: the normal
    matrix of the gradient layer, None = normal_matrix(basis), the committed camera's own"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, active_pixels=h * w, samples=0, shaded=0, gradients=0, hinge=0, w_borderline=0)
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
        r = rays(volume, org, d, rate, colors, alphas, tf_range, lo, hi, shading, light, intensity, material, basis[0], view, columns, spacing, origin,
                 vertex_centred, clip, sampler, camera_kind)
        rgba = (rgba + r["rgba"]).astype(F)
        layer = (layer + r["layer"]).astype(F)
        counters["rays"] += h * w
        counters["samples"] += int(r["steps"].sum())
        counters["shaded"] += int(r["shaded"].sum())
        counters["gradients"] += int(r["gradients"].sum())
        counters["hinge"] += int(r["hinge"].sum())
        counters["w_borderline"] += int(r["w_borderline"].sum())
        borderline |= r["borderline"]
    counters["borderline"] = borderline.reshape(h, w)
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
