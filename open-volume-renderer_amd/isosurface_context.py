"""The isosurface context of the HIP backend (include/ovr_hip.h, ovr_hip_set_isosurface_context) as a numpy model: the normative text.

In a context frame ONE walk both composites the unshaded emission-absorption march and finds, shades and composites every crossing of the committed isovalues,
each in its place along the ray.  Everything is float32, fma is a fused multiply-add, every other operation rounds on its own.  The ray, the box test and the
steps are the isosurface frame's (isosurface.py), which are the projection's (projection.py) and the march's; the side of a sample, the events of a step, the
refinement, the normal and the shadow walk are isosurface.py's; the classification is projection.py's, the box clipping.py's, the shade factor lighting.py's, the
opacity correction and its deterministic pow slice_context.py's: imported here, not restated.

Per pixel sample (world origin o, direction d):

    ray, steps  (t0, t1, hit) of the (clipped) box test, with the orthographic rule for ignored slabs; tx_0 = t0, ty_0 = fmin(t1, t0 + step),
                tm_i = 0.5 * (tx_i + ty_i), tx_{i+1} = ty_i, ty_{i+1} = fmin(tx_{i+1} + step, t1); s_i = the tap at to_object(fma(tm_i, d, o)).
    state       A = 0, C = 0, layer unset.  Step i exists while ty_i > tx_i and A < 0.9999: the march's loop condition, tested before every step.
    step i      1. events, if i >= 1 and side(s_{i-1}) != side(s_i): isosurface.events_of_step in its order; each event k is refined from the step's pair with
                   iso = iso_k (isosurface.refine), has the normal isosurface.normals gives at pos* and, under FULL, the shadow term of isosurface.py's translucent
                   shadow walk (cast by the level sets alone, with their opacities); c_k = the colour table at iso_k, under GRADIENT / FULL
                   clamp01(rgb * lighting.shade(...)).  Composite with the isovalue's own opacity alpha_k (the scale does not touch it):
                       tr = 1 - A;  C_ch = fma(tr * c_k_ch, alpha_k, C_ch);  A = fma(tr, alpha_k, A)
                   The ray's first event sets the layer (iso_k, t*_k, 1).  A >= 0.9999 behind an event ends the ray there: later events of the step and the
                   step's own volume sample are not taken.
                2. the volume sample, the march's under SHADE_NONE, operation for operation:
                       rgb, a_tf = projection.classify(s_i);  a = opacity_correction(a_tf, base, ty_i - tx_i);  a' = a * opacity_scale;  tr = 1 - A
                       C_ch = fma(tr * clamp01(rgb_ch), a', C_ch);  A = fma(tr, a', A)
                   (the surface of step i lies between tm_{i-1} and tm_i, in front of sample i: hence this order)
    sample      a = A; rgb = C / A per channel if A > 0, else 0.  The samples of a pixel are summed in order and multiplied by 1 / spp, as the isosurface frame's are.
    counters    samples = steps walked (every step fetches: nothing is range-skipped, on the primary walk or on a shadow walk); shaded_samples = events
                composited + volume samples composited with a' > 0; shadow_samples = the steps of all shadow walks.

Consequences (x * 1, fma(tr, 0, A) and fma(p, 0, C) with finite p are exact): with no crossing on any ray and scale 1 the frame is the unshaded march's bit for
bit; with an all-zero alpha table or scale 0 on a volume of finite voxels frame, layer, events and shadow steps are the translucent isosurface frame's bit for
bit (by its own identity the opaque frame's too); mode OFF is the isosurface frame.

Not done: a shaded context; volume shadows on the surfaces; ambient occlusion (a committed one is kept and not used); range and majorant skipping."""
import numpy as np

from . import clipping, isosurface, lighting, projection, slice_context
from .clipping import clamp01, fmin
from .isosurface import FULL, GRADIENT, NONE, events_of_step, normals, refine, side
from .lighting import fma
from .slice_context import opacity_correction

F = np.float32
OFF, VOLUME = 0, 1
ERT = slice_context.ERT     # the march's early-termination literal, 0.9999f
BASE = slice_context.BASE   # the march's `base`


def commit(mode, opacity_scale=1.0):
    """(mode, opacity_scale float32) as ovr_hip_set_isosurface_context stores them; ValueError where it returns EINVAL.  The scale is ignored, and stored as 1,
    in mode OFF"""
    if mode not in (OFF, VOLUME):
        raise ValueError("the isosurface context's mode is OFF or VOLUME")
    if int(mode) == OFF:
        return OFF, F(1)
    s = F(opacity_scale)
    if not (s >= 0 and s <= 1):
        raise ValueError("the isosurface context's opacity scale lies in [0, 1]")
    return VOLUME, s


def active(mode, n_isovalues, n_slices=0):
    """ovr_hip_get_isosurface_context().active: mode VOLUME, isovalues committed and no slices committed (slices keep their precedence)"""
    return int(mode == VOLUME and n_isovalues > 0 and n_slices == 0)


def context_rays(volume, org, direction, rate, iso, opacities, colors, alphas, tf_range, opacity_scale=1.0, spacing=(1, 1, 1), origin=(0, 0, 0),
                 vertex_centred=False, clip=None, shading=FULL, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL, eye=None, view=None,
                 sampler=None, camera_kind=0, border=1e-5):
    """world rays org, direction (n, 3) - the direction used as given - through the context walk: dict(n_events, A, steps (walked), shadow_steps, rgba (n, 4) of
    the sample, lit (volume samples composited with a' > 0), iso, t (the layer: the first event's), events (per ray a list of dict(i, k, t, normal, shadow, A -
    after the event -, pos, rgb)), order (per ray the composited items in order: ("event", i, k) and ("sample", i) with a' > 0), rays_hit; and for comparisons
    with a build whose pow differs in its last bit: borderline (a loop condition or an event's test met an A within `border` of 0.9999), borderline_event (such a
    ray that also has a crossing somewhere on [t0, t1]: layer and events may hang on that bit), hinge (for a borderline ray the steps from t0 to t1 plus all
    its crossings: the samples and shaded samples that hang on it), hinge_shadow (its crossings times the longest shadow walk of the box), borderline_steps
    (volume samples whose a' > 0 rests on the last bit of the pow: 0 < a <= 2^-22 with a != a_tf - slice_context.py's notion).
    opacities: one per isovalue as given (None: all ones, the opaque frame through the translucent text); eye: the camera position for the specular term
    (lighting.shade; default org); view: the orthographic camera's view vector"""
    scale = F(opacity_scale)
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    given = np.asarray(iso, F).ravel()
    alpha_k = isosurface.opacities_of(np.ones(given.size, F) if opacities is None else opacities, given)
    iso = isosurface.isovalues(given)
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    inv, wp = clipping.volume_constants(dims, spacing, origin, vertex_centred)
    lo, hi = ((0, 0, 0), (1, 1, 1)) if clip is None else clip
    if camera_kind:
        from . import camera
        t0, t1, hit = camera.hits(org, direction, inv, wp, lo, hi, camera_kind)
    else:
        t0, t1, hit = clipping.world_intervals(org, direction, inv, wp, lo, hi)
    m = len(t0)
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    step = F(1) / F(rate)
    raw_light = lighting.LITERAL_LIGHT if light is None else light
    L = lighting.normalize(np.asarray(raw_light, F))
    ka, kd, ks, shin = material
    eye = org if eye is None else np.broadcast_to(np.asarray(eye, F), org.shape)
    # the steps of the whole ray and their samples, as the projection forms them: what the walk below meets until it ends
    tm_all, count = projection.steps(t0, t1, step, hit)
    width = tm_all.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        po_all = clipping.to_object(fma(np.nan_to_num(tm_all)[:, :, None], direction[:, None, :], org[:, None, :]).reshape(-1, 3), inv, wp)
    s_all = tap(po_all).reshape(m, width) if width else np.zeros((m, 0), F)
    sd_all = side(s_all, iso)
    valid = np.arange(width)[None, :] < count[:, None]
    crossings = np.zeros(m, np.int64)
    if width > 1:
        crossings = (np.abs(sd_all[:, 1:] - sd_all[:, :-1]) * valid[:, 1:]).sum(1)
    diagonal = float(np.sqrt(((np.asarray(dims, np.float64) * np.asarray(spacing, np.float64)) ** 2).sum()))
    longest_shadow = int(np.ceil(diagonal * float(rate))) + 2

    A, C = np.zeros(m, F), np.zeros((m, 3), F)
    steps, lit, n_events, shadow_steps, borderline_steps = (np.zeros(m, np.int64) for _ in range(5))
    layer_iso, layer_t = np.zeros(m, F), np.zeros(m, F)
    events, order = [[] for _ in range(m)], [[] for _ in range(m)]
    near = np.zeros(m, bool)

    def take_events(idx, i, e):
        """event ordinal e of step i on the rays idx (each has one): composited into A, C; -> the rays that go on"""
        before, at = sd_all[idx, i - 1], sd_all[idx, i]
        k = np.array([list(events_of_step(int(b), int(a)))[e] for b, a in zip(before, at)], np.int64)
        o, d = org[idx], direction[idx]

        def tap_ray(t):
            with np.errstate(invalid="ignore", over="ignore"):
                return tap(clipping.to_object(fma(t[:, None], d, o), inv, wp))

        t, _, _ = refine(tap_ray, iso[k], tm_all[idx, i - 1], s_all[idx, i - 1], tm_all[idx, i], s_all[idx, i])
        with np.errstate(invalid="ignore", over="ignore"):
            pos = fma(t[:, None], d, o)
        po = clipping.to_object(pos, inv, wp)
        n_w = normals(tap, po, tap(po), dims, inv, vertex_centred) if shading != NONE else np.zeros((len(idx), 3), F)
        shadow, walked = np.zeros(len(idx), F), np.zeros(len(idx), np.int64)
        if shading == FULL:   # isosurface.py's translucent shadow walk: the steps from s0 + step, the opacities of the level sets crossed until A_s >= 0.9999
            Ld = np.broadcast_to(L, pos.shape)
            s0, s1, sbox = clipping.world_intervals(pos, Ld, inv, wp, lo, hi)
            stm, scount = projection.steps((s0 + step).astype(F), s1, step, sbox)
            if stm.shape[1] == 0:
                stm = np.zeros((len(idx), 1), F)
            with np.errstate(invalid="ignore", over="ignore"):
                spo = clipping.to_object(fma(np.nan_to_num(stm)[:, :, None], Ld[:, None, :], pos[:, None, :]).reshape(-1, 3), inv, wp)
            sw = isosurface.walk(tap(spo).reshape(stm.shape), scount, iso, None, alpha_k)
            shadow = np.array([row[-1][2] if row else F(0) for row in sw["events"]], F)
            walked = np.where(sbox, sw["walked"], 0)
        rgb = projection.classify(iso[k], colors, np.zeros(2, F), *tf_range)[:, :3]
        if shading != NONE:
            f = lighting.shade(n_w, pos, shadow, L, eye[idx], ka, kd, ks, shin, intensity, view=view)
            with np.errstate(invalid="ignore", over="ignore"):
                rgb = clamp01((rgb * f[:, None]).astype(F))
        tr = (F(1) - A[idx]).astype(F)
        C[idx] = fma((tr[:, None] * rgb).astype(F), alpha_k[k][:, None], C[idx])
        A[idx] = fma(tr, alpha_k[k], A[idx])
        first = n_events[idx] == 0
        layer_iso[idx], layer_t[idx] = np.where(first, iso[k], layer_iso[idx]), np.where(first, t, layer_t[idx])
        n_events[idx] += 1
        shadow_steps[idx] += walked
        for j, r in enumerate(idx):
            events[r].append(dict(i=int(i), k=int(k[j]), t=t[j], normal=n_w[j], shadow=shadow[j], A=A[r], pos=pos[j], rgb=rgb[j]))
            order[r].append(("event", int(i), int(k[j])))
        near[idx] |= np.abs(A[idx].astype(np.float64) - float(ERT)) <= border
        return A[idx] < ERT

    with np.errstate(invalid="ignore", over="ignore"):
        tx = t0.copy()
        ty = fmin(t1, (t0 + step).astype(F))
        live = hit.copy()
        i = 0
        while True:
            near |= live & (ty > tx) & (np.abs(A.astype(np.float64) - float(ERT)) <= border)
            live = live & (ty > tx) & (A < ERT)
            idx = np.flatnonzero(live)
            if not idx.size:
                break
            steps[idx] += 1
            open_ = np.ones(idx.size, bool)
            if i >= 1:
                n_ev = np.abs(sd_all[idx, i] - sd_all[idx, i - 1])
                for e in range(isosurface.MAX_ISOVALUES):
                    sel = open_ & (e < n_ev)
                    if not sel.any():
                        break
                    open_[sel] = take_events(idx[sel], i, e)
            live[idx[~open_]] = False   # saturated behind an event: the ray ends there, the step's own sample is not taken
            idx = idx[open_]
            x, y = tx[idx], ty[idx]
            c = projection.classify(s_all[idx, i], colors, alphas, *tf_range)
            a_tf = c[:, 3]
            a = opacity_correction(a_tf, BASE, (y - x).astype(F))
            a1 = (a * scale).astype(F)
            tr = (F(1) - A[idx]).astype(F)
            C[idx] = fma((tr[:, None] * clamp01(c[:, :3])).astype(F), a1[:, None], C[idx])
            A[idx] = fma(tr, a1, A[idx])
            lit[idx] += a1 > 0
            borderline_steps[idx] += (a_tf > 0) & (a <= F(2.0 ** -22)) & (a != a_tf)
            for r in idx[a1 > 0]:
                order[r].append(("sample", i))
            tx = np.where(live, ty, tx).astype(F)
            ty = np.where(live, fmin((tx + step).astype(F), t1), ty).astype(F)
            i += 1
    rgba = np.zeros((m, 4), F)
    pos_a = A > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rgba[:, :3] = np.where(pos_a[:, None], (C / np.where(pos_a, A, F(1))[:, None]).astype(F), F(0))
    rgba[:, 3] = A
    near_event = near & (crossings > 0)
    return dict(n_events=n_events, A=A, steps=steps, shadow_steps=shadow_steps, rgba=rgba, lit=lit, iso=layer_iso, t=layer_t, events=events, order=order,
                rays_hit=hit, borderline_steps=borderline_steps, borderline=near, borderline_event=near_event, hinge=np.where(near, count + crossings, 0),
                hinge_shadow=np.where(near, crossings * longest_shadow, 0))


def frame(volume, basis, size, rate, iso, opacities, colors, alphas, tf_range, opacity_scale=1.0, shading=FULL, light=None, intensity=1.0,
          material=lighting.REFERENCE_MATERIAL, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, spp=1, noise=None,
          frame_index=1, camera_kind=0):
    """one context frame: rgba (H, W, 4), layer (H, W, 3) and counters (rays, active_pixels, samples = steps walked, shaded = events + lit volume samples,
    events, lit, shadow_steps; hinge, hinge_shadow, borderline_steps and the two borderline pixel masks, see context_rays).  The arguments are isosurface.frame's, with the
    alpha table and the scale"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, active_pixels=h * w, samples=0, shaded=0, events=0, lit=0, shadow_steps=0, hinge=0, hinge_shadow=0, borderline_steps=0)
    borderline, borderline_event = np.zeros(h * w, bool), np.zeros(h * w, bool)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    for j in range(spp):
        xi = None if noise is None else projection.blue_noise_variates(noise, w, h, frame_index, spp, j)
        d = projection.pixel_rays(basis, w, h, xi).reshape(-1, 3)
        view = None
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
            view = camera.view_vector(basis) if camera_kind == camera.ORTHOGRAPHIC else None
        r = context_rays(volume, org, d, rate, iso, opacities, colors, alphas, tf_range, opacity_scale, spacing, origin, vertex_centred, clip, shading, light,
                         intensity, material, basis[0], view, sampler, camera_kind)
        rgba = (rgba + r["rgba"]).astype(F)
        has = r["n_events"] > 0
        layer = (layer + np.where(has[:, None], np.stack([r["iso"], r["t"], np.ones(h * w, F)], 1), F(0))).astype(F)
        counters["rays"] += h * w
        counters["samples"] += int(r["steps"].sum())
        counters["events"] += int(r["n_events"].sum())
        counters["lit"] += int(r["lit"].sum())
        counters["shaded"] += int(r["n_events"].sum() + r["lit"].sum())
        counters["shadow_steps"] += int(r["shadow_steps"].sum())
        counters["hinge"] += int(r["hinge"].sum())
        counters["hinge_shadow"] += int(r["hinge_shadow"].sum())
        counters["borderline_steps"] += int(r["borderline_steps"].sum())
        borderline |= r["borderline"]
        borderline_event |= r["borderline_event"]
    counters["borderline"], counters["borderline_event"] = borderline.reshape(h, w), borderline_event.reshape(h, w)
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
