"""The slice frames of the HIP backend (include/ovr_hip.h, ovr_hip_set_slices) as a numpy model: the normative text.

A slice frame shows the volume on up to MAX_SLICES = 4 cut planes or thick slabs.  Everything is float32, fma is a fused multiply-add, every other operation
rounds on its own.  The ray, the box test, the steps, the tap, the three reductions, the range-skipping rule and the classification are projection.py's (and
clipping.py's, camera.py's): imported here, not restated.

Host (`commit`): per slice the caller gives a world point, a world normal of any length, a thickness (world units along the normal; 0: a plane, > 0: a slab
centred on the plane, +inf: the whole box) and a mode (projection.MAXIMUM / MINIMUM / MEAN, read only while thickness > 0).

    n    = normal / |normal| in float64, each component rounded to float32
    c    = float32(dot(n, point)) - formed in float64 from the ROUNDED n, rounded once
    half = 0.5f * thickness

Per ray (world origin o, direction d; (t0, t1, hit) the projection's box test, the clipped one while a clip box is committed) and slice k:

    dn = fma(n.x, d.x, fma(n.y, d.y, n.z * d.z))
    e  = fma(n.x, o.x, fma(n.y, o.y, n.z * o.z)) - c

    plane   ts = (-e) / dn;  met iff hit and dn != 0 and ts >= t0 and ts <= t1 (a NaN meets nothing);  key t_k = ts
    slab    dn != 0: a = (-half - e) / dn, b = (half - e) / dn, swapped if a > b; ta = fmax(t0, a), tb = fmin(t1, b)
            dn == 0: (ta, tb) = (t0, t1) if |e| <= half, otherwise not met
            met iff hit and tb > ta;  key t_k = ta
            (thickness = +inf: a = -inf, b = +inf whatever the finite e and dn != 0 are, and |e| <= inf: (ta, tb) = (t0, t1) bit for bit - the whole-box slab
            walks the projection's interval)

Winner: the met slice with the smallest key; of equal keys the lowest index.  ONLY the winner is sampled:

    plane   v = the trilinear tap (projection.sample) at to_object(fma(ts, d, o)); one step
    slab    projection.steps on (ta, tb) with step = 1 / sampling rate, every sample at to_object(fma(tm_i, d, o)), projection.reduce of the slice's mode.
            A winning slab without a step counts as not met - the next nearest slice is NOT tried.

Pixel sample: nothing met: rgba = 0, layer = 0.  Otherwise rgb = projection.classify's colour at v (clamped), a = 1 - a slice is opaque, the alpha table is not
read - and the layer is (v, t_k, k + 1).  The samples of a pixel are summed in order and multiplied by 1 / spp, as the projection's are.

Range skipping: a MAXIMUM or MINIMUM slab drops fetches by projection.reduce_skipping's rule (slack, tap_cell, the bound from the rounds before the step's own).
Planes and MEAN slabs fetch everything."""
import numpy as np

from . import clipping, projection
from .clipping import fmax, fmin
from .lighting import fma
from .projection import MAXIMUM, MEAN, MINIMUM

F = np.float32
MAX_SLICES = 4


# ---- host ------------------------------------------------------------------------------------------------------------------------------
def _as_tuple(s):
    if isinstance(s, dict):
        return s["point"], s["normal"], s.get("thickness", 0.0), s.get("mode", MAXIMUM)
    s = tuple(s)
    return s[0], s[1], (s[2] if len(s) > 2 else 0.0), (s[3] if len(s) > 3 else MAXIMUM)


def commit(slices):
    """the caller's slices (dicts or (point, normal, thickness = 0, mode = MAXIMUM) tuples) -> the committed values: a list of dict(n (3,) float32, c, half,
    thickness float32, mode int).  ValueError where ovr_hip_set_slices returns EINVAL"""
    slices = [] if slices is None else list(slices)
    if len(slices) > MAX_SLICES:
        raise ValueError("between 0 and 4 slices")
    out = []
    for s in slices:
        point, normal, thickness, mode = _as_tuple(s)
        point, normal = np.asarray(point, F), np.asarray(normal, F)
        thickness = F(thickness)
        if point.shape != (3,) or normal.shape != (3,) or not np.isfinite(point).all():
            raise ValueError("a slice's point must be finite")
        n64 = normal.astype(np.float64)
        length = np.sqrt((n64 * n64).sum())
        if not np.isfinite(normal).all() or not (length > 0.0) or not np.isfinite(length):
            raise ValueError("a slice's normal cannot be normalised")
        n = (n64 / length).astype(F)
        if not np.isfinite(n).all() or not n.any():
            raise ValueError("a slice's normal cannot be normalised")
        if not thickness >= 0:
            raise ValueError("a slice's thickness is 0, positive or +inf")
        if thickness > 0 and mode not in (MAXIMUM, MINIMUM, MEAN):
            raise ValueError("a slab's mode is MAXIMUM, MINIMUM or MEAN")
        c = F((n.astype(np.float64) * point.astype(np.float64)).sum())
        out.append(dict(n=n, c=c, half=F(F(0.5) * thickness), thickness=thickness, mode=int(mode)))
    return out


# ---- the slice stage -------------------------------------------------------------------------------------------------------------------
def meet(s, org, direction, t0, t1, hit):
    """one committed slice against rays: (met (n,), key (n,), ta (n,), tb (n,)); for a plane ta = tb = ts"""
    n, c, half = s["n"], s["c"], s["half"]
    o, d = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    t0, t1, hit = np.asarray(t0, F), np.asarray(t1, F), np.asarray(hit, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dn = fma(n[0], d[:, 0], fma(n[1], d[:, 1], (n[2] * d[:, 2]).astype(F)))
        e = (fma(n[0], o[:, 0], fma(n[1], o[:, 1], (n[2] * o[:, 2]).astype(F))) - c).astype(F)
        if not s["thickness"] > 0:
            ts = ((-e).astype(F) / dn).astype(F)
            met = hit & (dn != 0) & (ts >= t0) & (ts <= t1)
            return met, ts, ts, ts
        a = ((-half - e).astype(F) / dn).astype(F)
        b = ((half - e).astype(F) / dn).astype(F)
        swap = a > b
        a, b = np.where(swap, b, a), np.where(swap, a, b)
        ta, tb = fmax(t0, a), fmin(t1, b)
        par = dn == 0
        inside = np.abs(e) <= half
        ta, tb = np.where(par, t0, ta).astype(F), np.where(par, t1, tb).astype(F)
        met = hit & (tb > ta) & (~par | inside)
    return met, ta, ta, tb


def winner(committed, org, direction, t0, t1, hit):
    """(k (n,) - the winning slice's index or -1 -, key, ta, tb of the winner)"""
    m = len(np.asarray(t0).ravel())
    k = np.full(m, -1, np.int64)
    key, wa, wb = np.zeros(m, F), np.zeros(m, F), np.zeros(m, F)
    for i, s in enumerate(committed):
        met, t, ta, tb = meet(s, org, direction, t0, t1, hit)
        with np.errstate(invalid="ignore"):
            take = met & ((k < 0) | (t < key))
        k = np.where(take, i, k)
        key, wa, wb = np.where(take, t, key).astype(F), np.where(take, ta, wa).astype(F), np.where(take, tb, wb).astype(F)
    return k, key, wa, wb


# ---- rays and frames -------------------------------------------------------------------------------------------------------------------
def slice_rays(volume, org, direction, rate, slices, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, skipping=False,
               camera_kind=0):
    """world rays org, direction (n, 3) - the direction used as given - against `slices` (the caller's values, or commit()'s) -> dict(k (the winner's index + 1,
    0: nothing met), v, t, steps, fetched, met, rays_hit): what ovr_hip_slice_floats returns, and the fetches.  The arguments are projection.project_rays'"""
    committed = slices if slices and isinstance(slices[0], dict) and "half" in slices[0] else commit(slices)
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    inv, wp = clipping.volume_constants(dims, spacing, origin, vertex_centred)
    lo, hi = ((0, 0, 0), (1, 1, 1)) if clip is None else clip
    if camera_kind:
        from . import camera
        t0, t1, hit = camera.hits(org, direction, inv, wp, lo, hi, camera_kind)
    else:
        t0, t1, hit = clipping.world_intervals(org, direction, inv, wp, lo, hi)
    k, key, ta, tb = winner(committed, org, direction, t0, t1, hit)
    m = len(k)
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    v, steps, fetched = np.zeros(m, F), np.zeros(m, np.int64), np.zeros(m, np.int64)
    ranges = None
    for i, s in enumerate(committed):
        mine = np.flatnonzero(k == i)
        if not mine.size:
            continue
        o, d = org[mine], direction[mine]
        if not s["thickness"] > 0:
            with np.errstate(invalid="ignore", over="ignore"):
                po = clipping.to_object(fma(key[mine][:, None], d, o), inv, wp)
            v[mine] = tap(po)
            steps[mine] = fetched[mine] = 1
            continue
        tm, count = projection.steps(ta[mine], tb[mine], F(1) / F(rate))
        width = tm.shape[1]
        with np.errstate(invalid="ignore", over="ignore"):
            pos = fma(np.nan_to_num(tm)[:, :, None], d[:, None, :], o[:, None, :])
            po = clipping.to_object(pos.reshape(-1, 3), inv, wp)
        smp = tap(po).reshape(mine.size, width)
        if skipping and s["mode"] != MEAN:
            if ranges is None:
                ranges = projection.macrocell_ranges(vol)
            i0, _ = projection.tap_coordinates(po, dims, vertex_centred)
            cell = projection.tap_cell(i0, dims)
            rng = ranges[cell[:, 2], cell[:, 1], cell[:, 0]].reshape(mine.size, width, 2)
            sv, _, sf = projection.reduce_skipping(smp, tm, count, rng[..., 0], rng[..., 1], s["mode"])
        else:
            sv, _ = projection.reduce(smp, tm, count, s["mode"])
            sf = count
        v[mine], steps[mine], fetched[mine] = sv, count, sf
    met = (k >= 0) & (steps > 0)   # a winning slab without a step counts as not met
    z = F(0)
    return dict(k=np.where(met, k + 1, 0), v=np.where(met, v, z).astype(F), t=np.where(met, key, z).astype(F), steps=np.where(met, steps, 0),
                fetched=np.where(met, fetched, 0), met=met, rays_hit=hit)


def frame(volume, basis, size, rate, slices, colors, tf_range, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None,
          skipping=False, spp=1, noise=None, frame_index=1, camera_kind=0):
    """one slice frame: rgba (H, W, 4), layer (H, W, 3) and counters (rays, active_pixels, steps, fetched).  The arguments are projection.frame's, without the
    alpha table: a slice is opaque"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    committed = commit(slices)
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, active_pixels=h * w, steps=0, fetched=0)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    for j in range(spp):
        xi = None if noise is None else projection.blue_noise_variates(noise, w, h, frame_index, spp, j)
        d = projection.pixel_rays(basis, w, h, xi).reshape(-1, 3)
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
        r = slice_rays(volume, org, d, rate, committed, spacing, origin, vertex_centred, clip, sampler, skipping, camera_kind)
        m = r["met"]
        c = projection.classify(r["v"], colors, np.ones(2, F), *tf_range)
        c[:, 3] = F(1)
        rgba = (rgba + np.where(m[:, None], c, F(0))).astype(F)
        layer = (layer + np.where(m[:, None], np.stack([r["v"], r["t"], r["k"].astype(F)], 1), F(0))).astype(F)
        counters["rays"] += h * w
        counters["steps"] += int(r["steps"].sum())
        counters["fetched"] += int(r["fetched"].sum())
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
