"""The slice context of the HIP backend (include/ovr_hip.h, ovr_hip_set_slice_context) as a numpy model: the normative text.

A context frame is a slice frame (slices.py) in which the unshaded emission-absorption march runs from the ray's entry into the box up to the winning slice;
the opaque slice is composited behind it.  Everything is float32, fma is a fused multiply-add, every other operation rounds on its own.  The ray, the box test
and the slice stage are slices.py's, the tap and the classification projection.py's, the box clipping.py's, the deterministic log2 / exp2 pair lighting.py's:
imported here, not restated.

Per pixel sample (world origin o, direction d):

    1. (t0, t1, hit) and the winner (k, key, ta, tb) exactly as slices.py forms them; a ray that is not hit gives zeros.  The winner counts as met under
       slices.py's rule ("a winning slab without a step counts as not met").
    2. the cut: tc = key if a slice is met, else t1.
    3. the context march - the primary loop of the unshaded march with tc in t1's place, operation for operation:
           alpha = 0, C = 0, tx = t0, ty = fmin(tc, t0 + step)
           while ty > tx and alpha < 0.9999:
               tm  = 0.5 * (tx + ty)
               s   = the tap at to_object(fma(tm, d, o))
               rgb, a_tf = the march's classification of s (projection.classify: the colour table's and the alpha table's nodal lerp)
               a   = opacity_correction(a_tf, base, ty - tx)          base = 1; adj = base * dt; |adj - 1| < 1e-7 keeps a_tf, otherwise
                                                                      clamp01(1 - pow(1 - a_tf, adj)) with pow(x, y) = det_exp2(y * det_log2(x))
               a'  = a * opacity_scale
               tr  = 1 - alpha
               C_ch  = fma(tr * clamp01(rgb_ch), a', C_ch)
               alpha = fma(tr, a', alpha)
               tx = ty, ty = fmin(tx + step, tc)
    4. the slice behind it, composited iff one is met and alpha < 0.9999 (the loop's own condition: a saturated ray neither taps a plane nor walks a slab):
           v = the slice frame's value of the winner; c = clamp01 of the projection's colour at v
           tr = 1 - alpha;  C_ch = fma(tr * c_ch, 1, C_ch);  alpha = fma(tr, 1, alpha)
       the layer is (v, t_k, k + 1) when the slice was composited, else (0, 0, 0).
    5. the sample: a = alpha; rgb = C / a per channel if a > 0, else 0 - the march's un-premultiplied pixel.  The samples of a pixel are summed in order and
       multiplied by 1 / spp, as the slice frame's are.
    6. counters: samples = context steps fetched + the composited winner's fetched taps; shaded_samples = context steps with a' > 0; nothing is skipped.

Consequences (x * 1 and fma(1 * c, 1, 0) are exact): with no slice met and scale 1 the sample is the unshaded march's bit for bit; with an all-zero alpha table
or scale 0 frame and layer are the slice frame's bit for bit; mode OFF is the slice frame."""
import numpy as np

from . import clipping, projection, slices
from .clipping import clamp01, fmin
from .lighting import det_exp2, det_log2, fma

F = np.float32
OFF, FRONT = 0, 1
ERT = F(0.9999)            # the march's early-termination literal
NEARLY_EQUAL_EPS = F(1e-7)  # the march's nearly_equal
BASE = F(1)                 # the march's `base`


def commit(mode, opacity_scale=1.0):
    """(mode, opacity_scale float32) as ovr_hip_set_slice_context stores them; ValueError where it returns EINVAL.  The scale is ignored, and stored as 1, in
    mode OFF"""
    if mode not in (OFF, FRONT):
        raise ValueError("the slice context's mode is OFF or FRONT")
    if int(mode) == OFF:
        return OFF, F(1)
    s = F(opacity_scale)
    if not (s >= 0 and s <= 1):
        raise ValueError("the slice context's opacity scale lies in [0, 1]")
    return FRONT, s


def det_pow(x, y):
    """lighting.det_exp2(y * det_log2(x)) - the exact-parity build's pair - for x in [0, 1]: log2(0) = -inf"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pos = x > 0
        l = np.where(pos, det_log2(np.where(pos, x, F(1)).astype(F)), np.where(x == 0, F(-np.inf), F(np.nan))).astype(F)
        return det_exp2((y * l).astype(F))


def opacity_correction(a, base, dt):
    a, dt = np.asarray(a, F), np.asarray(dt, F)
    with np.errstate(invalid="ignore", over="ignore"):
        adj = (F(base) * dt).astype(F)
        keep = np.abs((adj - F(1)).astype(F)) < NEARLY_EQUAL_EPS
        c = clamp01((F(1) - det_pow((F(1) - a).astype(F), adj)).astype(F))
        return np.where(keep, a, c).astype(F)


def context_rays(volume, org, direction, rate, slice_list, colors, alphas, tf_range, opacity_scale=1.0, spacing=(1, 1, 1), origin=(0, 0, 0),
                 vertex_centred=False, clip=None, sampler=None, camera_kind=0, border=1e-5):
    """world rays org, direction (n, 3) - the direction used as given - against the slices with the context in front: dict(k (the composited slice's index + 1
    or 0), v, t, steps (context steps taken), rgba (n, 4) of the sample, fetched (the composited winner's taps), shaded (context steps with a' > 0),
    alpha_front (alpha before the slice), met (a slice is met, composited or not), rays_hit, borderline_steps (context steps whose a' > 0 rests on the last
    bit of the pow: 0 < a <= 2^-22 with a != a_tf), and - for comparisons with a build whose pow differs in its last bit - borderline (a loop condition or the
    slice's test met an alpha within `border` of 0.9999: whether the ray went on there rests on that bit), borderline_front (the slice's test alone: whether
    the slice is composited rests on it) and hinge (the samples that hang on it: the steps
    from t0 to the cut without early termination + the winner's taps))"""
    scale = F(opacity_scale)
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    committed = slice_list if slice_list and isinstance(slice_list[0], dict) and "half" in slice_list[0] else slices.commit(slice_list)
    inv, wp = clipping.volume_constants(dims, spacing, origin, vertex_centred)
    lo, hi = ((0, 0, 0), (1, 1, 1)) if clip is None else clip
    if camera_kind:
        from . import camera
        t0, t1, hit = camera.hits(org, direction, inv, wp, lo, hi, camera_kind)
    else:
        t0, t1, hit = clipping.world_intervals(org, direction, inv, wp, lo, hi)
    m = len(t0)
    if committed:
        sr = slices.slice_rays(vol, org, direction, rate, committed, spacing, origin, vertex_centred, clip, sampler, False, camera_kind)
    else:
        z = np.zeros(m, np.int64)
        sr = dict(k=z, v=np.zeros(m, F), t=np.zeros(m, F), steps=z, fetched=z, met=np.zeros(m, bool))
    met = sr["met"]
    tc = np.where(met, sr["t"], t1).astype(F)
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    step = F(1) / F(rate)
    alpha, C = np.zeros(m, F), np.zeros((m, 3), F)
    steps, shaded, borderline = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    near = np.zeros(m, bool)
    with np.errstate(invalid="ignore", over="ignore"):
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
            po = clipping.to_object(fma(tm[:, None], direction[idx], org[idx]), inv, wp)
            c = projection.classify(tap(po), colors, alphas, *tf_range)
            a_tf = c[:, 3]
            a = opacity_correction(a_tf, BASE, (y - x).astype(F))
            a1 = (a * scale).astype(F)
            tr = (F(1) - alpha[idx]).astype(F)
            C[idx] = fma((tr[:, None] * clamp01(c[:, :3])).astype(F), a1[:, None], C[idx])
            alpha[idx] = fma(tr, a1, alpha[idx])
            steps[idx] += 1
            shaded[idx] += a1 > 0
            borderline[idx] += (a_tf > 0) & (a <= F(2.0 ** -22)) & (a != a_tf)
            tx = np.where(live, ty, tx).astype(F)
            ty = np.where(live, fmin((tx + step).astype(F), tc), ty).astype(F)
    alpha_front = alpha.copy()
    near_front = met & (np.abs(alpha.astype(np.float64) - float(ERT)) <= border)
    near |= near_front
    _, to_cut = projection.steps(t0, tc, step, hit)
    comp = met & (alpha < ERT)
    cs = clamp01(projection.classify(sr["v"], colors, np.ones(2, F), *tf_range)[:, :3])
    tr = (F(1) - alpha).astype(F)
    C = np.where(comp[:, None], fma((tr[:, None] * cs).astype(F), F(1), C), C).astype(F)
    alpha = np.where(comp, fma(tr, F(1), alpha), alpha).astype(F)
    rgba = np.zeros((m, 4), F)
    pos = alpha > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rgba[:, :3] = np.where(pos[:, None], (C / np.where(pos, alpha, F(1))[:, None]).astype(F), F(0))
    rgba[:, 3] = alpha
    z = F(0)
    return dict(k=np.where(comp, sr["k"], 0), v=np.where(comp, sr["v"], z).astype(F), t=np.where(comp, sr["t"], z).astype(F), steps=steps, rgba=rgba,
                fetched=np.where(comp, sr["fetched"], 0), shaded=shaded, alpha_front=alpha_front, met=met, rays_hit=hit, borderline_steps=borderline, borderline=near, borderline_front=near_front,
                hinge=np.where(near, to_cut + np.where(met, sr["fetched"], 0), 0))


def frame(volume, basis, size, rate, slice_list, colors, alphas, tf_range, opacity_scale=1.0, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False,
          clip=None, sampler=None, spp=1, noise=None, frame_index=1, camera_kind=0):
    """one context frame: rgba (H, W, 4), layer (H, W, 3) and counters (rays, active_pixels, samples, shaded, context_steps, borderline_steps; hinge and
    the two borderline pixel masks, see context_rays).  The arguments
    are slices.frame's, with the alpha table and the scale"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    committed = slices.commit(slice_list)
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, active_pixels=h * w, samples=0, shaded=0, context_steps=0, borderline_steps=0, hinge=0)
    borderline, borderline_front = np.zeros(h * w, bool), np.zeros(h * w, bool)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    for j in range(spp):
        xi = None if noise is None else projection.blue_noise_variates(noise, w, h, frame_index, spp, j)
        d = projection.pixel_rays(basis, w, h, xi).reshape(-1, 3)
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
        r = context_rays(volume, org, d, rate, committed, colors, alphas, tf_range, opacity_scale, spacing, origin, vertex_centred, clip, sampler, camera_kind)
        rgba = (rgba + r["rgba"]).astype(F)
        layer = (layer + np.stack([r["v"], r["t"], r["k"].astype(F)], 1)).astype(F)
        counters["rays"] += h * w
        counters["context_steps"] += int(r["steps"].sum())
        counters["samples"] += int(r["steps"].sum() + r["fetched"].sum())
        counters["shaded"] += int(r["shaded"].sum())
        counters["borderline_steps"] += int(r["borderline_steps"].sum())
        counters["hinge"] += int(r["hinge"].sum())
        borderline |= r["borderline"]
        borderline_front |= r["borderline_front"]
    counters["borderline"], counters["borderline_front"] = borderline.reshape(h, w), borderline_front.reshape(h, w)
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
