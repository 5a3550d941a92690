"""The isosurfaces of the HIP backend (include/ovr_hip.h, ovr_hip_set_isosurfaces) as a numpy model: the normative text.

Opaque, shaded, hard-shadowed level sets of the resident volume for up to four isovalues iso_0 < iso_1 < ..., drawn in the march's place.  Everything is
float32; fma is lighting.fma, every other operation rounds on its own.  The ray, the steps tm_i and the samples s_i are the projection's (projection.py:
`pixel_rays`, `steps`, `sample`), with the clipped box test while a clip box is committed.

Side       side(s) = #{k : iso_k <= s}; a NaN compares false, its side is 0.
Hit        the first step i >= 1 with side(s_{i-1}) != side(s_i).  No caps: a box face or a clip face is no surface.  Rising (the side grows): k* = side(s_{i-1}),
           the lowest isovalue crossed; falling: k* = side(s_{i-1}) - 1, the highest.  iso = iso_{k*}.  The walk ends at step i: steps walked = i + 1 on a hit, n
           on a miss.
Refinement two rounds of four points - what four lanes per ray evaluate at once.  From (ta, sa) = (tm_{i-1}, s_{i-1}), (tb, sb) = (tm_i, s_i), in(x) = (iso <= x):
           a round taps q_j at p_j = fma(c_j, tb - ta, ta), c = (0.2f, 0.4f, 0.6f, 0.8f); of the sequence sa, q_1 .. q_4, sb the first consecutive pair whose `in`
           differs becomes the new (ta, sa), (tb, sb) (in(sa) != in(sb) holds for the hit's pair and is kept by every round).  Then
           t* = fmin(fmax(fma((iso - sa) / (sb - sa), tb - ta, ta), ta), tb), pos* = fma(t*, dir, org), s* = the tap at pos*.
Normal     shade_request's forward difference at po* = to_object(pos*): per axis d = -g if po* + g > 1 else g (g = one voxel in object space), (tap(po* + d e) - s*) / d;
           then normalize, negate, times otw_it (= inv_scale), normalize.  normalize = lighting.normalize.  (The product multiplies with 1 / g and normalises with
           v_rsq_f32, as in the march; the exact-parity build is this text.)
Shadow     under OVR_HIP_SHADE_FULL only: the ray pos* + t * light through the (clipped) box, (t0, t1, hit) from (0, FLT_MAX); its steps are the projection's
           recurrence from tx_0 = t0 + step (t0 = 0 for a point inside the box: the first two samples sit at 1.5 and 2.5 step); shadow = 1 iff two consecutive
           shadow samples differ in side, else 0; the walk ends at the first such pair, nothing is refined.
Pixel      a miss: zeros.  A hit: rgb = the colour table at iso (projection.classify; the alpha table is not read); under NONE as it is, under GRADIENT / FULL
           clamp01(rgb * lighting.shade(n_w, pos*, shadow, ...)) with the committed light and material; a = 1; the layer is (iso, t*, 1).  The samples of a
           pixel are summed in order and multiplied by 1 / spp.
Skipping   (primary and shadow walks, while range skipping is on) with [lo, hi] the value range of the step's tap_cell, S = projection.slack(lo, hi), a = lo - S,
           b = hi + S: the step's fetch is dropped iff every k has iso_k < a or iso_k > b (a NaN bound proves nothing); its side is then #{k : iso_k < a} - the
           side of every sample the cell can produce, by the bound of DESIGN.md section 16.  The two samples of the hit's pair are always taken (for the
           refinement: a tap of its own at tm_{i-1} and tm_i, the walk's bits), whether the walk fetched them or not.
Counters   samples / skipped_samples = the walked steps whose fetch the WALK made / dropped (their sum: the steps walked); shaded_samples = hits; shadow_samples /
           skipped_shadow_samples = the same of the shadow walks.  Refinement, end-point and gradient taps are not counted.

Translucent (ovr_hip_set_isosurface_layers with an opacity below 1): each isovalue has an opacity alpha_k in (0, 1].
Events     every step i >= 1 with side(s_{i-1}) != side(s_i) holds one event per isovalue crossed, in the order the ray meets them: rising from side a to b > a
           k = a ... b - 1, falling to b < a k = a - 1 ... b.  The opaque hit is the first event of the first such step.  Each event is refined from the step's own
           pair with iso = iso_k (in(sa) != in(sb) holds for every crossed k), and shaded and shadowed as the hit is; c_k = its colour (clamp01(rgb * shade)).
Composite  the march's recurrence (oracle/ovr_oracle.c:608-615) from A = 0, C = 0: tr = 1 - A, C_ch = fma(tr * c_ch, alpha_k, C_ch), A = fma(tr, alpha_k, A).  The
           first event sets the layer.  A >= 0.9999f behind an event ends the ray there (later events of the step are not taken; steps walked = i + 1), else the
           walk goes on with step i + 1 whose predecessor is step i.  Sample: rgb = C / A per channel, a = A; zeros without an event.
Shadow     today's shadow ray and steps; A_s = fma(1 - A_s, alpha_k, A_s) over its events until A_s >= 0.9999f; shadow = A_s.
Counters   steps walked count once however many events they hold; shaded_samples = events composited; the shadow counters sum the shadow walks of all events.
With every alpha_k = 1 the first event gives C = c, A = 1 and the shadow 1.0f: the opaque text above, bit for bit.

Ambient occlusion (ovr_hip_set_ambient_occlusion(K, R)): under GRADIENT / FULL every event casts K occlusion walks into the hemisphere that
faces the viewer; K in 0 ... 16, R > 0 in world units of t (inf: the whole box).  K = 0: the text above.
Table      D[m][j], m = 0 ... 15, j = 0 ... K - 1 (`ao_directions`): in float64 r2 = (j + 0.5) / K, phi = 2 pi (j g + m / 16), g = 0.6180339887498949,
           (sqrt(r2) cos phi, sqrt(r2) sin phi, sqrt(1 - r2)), each component rounded to float32: cosine-weighted, z along the normal, sixteen rotations.
Rotation   sample k of frame frame_index (1-based) at pixel (x, y): m = ((x & 3) + 4 (y & 3) + (frame_index - 1) spp + k) & 15 (`ao_rotation`).
Normal     N = n_w if lighting.dot(n_w, dir) <= 0 else -n_w, dir the event's primary ray (a NaN normal stays NaN; its walks miss the box: O = 0).
Frame      Duff et al.'s basis, every operation on its own: s = copysign(1, N.z), a = -1 / (s + N.z), b = (N.x N.y) a,
           T = (1 + ((s N.x) N.x) a, s b, -(s N.x)), B = (b, s + (N.y N.y) a, -N.y).
Ray j      d_c = fma(x, T_c, fma(y, B_c, z N_c)) per component with (x, y, z) = D[m][j]; not renormalised.
Walk       the translucent shadow walk with d_j in the light's place: (a0, a1, hit) from the (clipped) box test of pos* + t d_j from (0, FLT_MAX), a1 = fmin(a1, R),
           steps from a0 + step, A_j = fma(1 - A_j, alpha_k, A_j) over its events until A_j >= 0.9999f or its last step; skipping as the shadow walk; nothing refined.
Shade      S = A_0 + ... + A_{K-1} in that order, O = S / (float)K; the event's shade factor is lighting.shade with ambient = ka * (1 - O).  O = 0: ka, today's bits.
Opaque     a frame without opacities runs this text with all-ones opacities (the identity above: the opaque frame apart from the ambient term).
Counters   the AO walks' steps are reported apart (ao_steps, ao_fetched); the product adds their fetched steps to shadow_samples and the dropped ones to
           skipped_shadow_samples.
This issue left open, fixed here: the operation order of the basis (above); a direction d_j for which the box test fails contributes A_j = 0; under NONE nothing
is cast; the known-answer entry casts under full shading whatever mode is committed.

The 8-bit voxel types: the product filters the stored integers and normalises once behind the filter (s = filter(raw) * (1 / 255)), the exact-parity build and
projection.sample normalise voxel by voxel.  `product_sampler` restates the former, so that hit, isovalue, t* and the steps walked of the product are this model's
bits too."""
import numpy as np

from . import clipping, lighting
from .clipping import clamp01, fmax, fmin
from .lighting import fma
from .projection import blue_noise_variates, classify, macrocell_ranges, pixel_rays, sample, slack, steps, tap_cell, tap_coordinates

F = np.float32
MAX_ISOVALUES = 4
NONE, GRADIENT, FULL = 0, 1, 2
C = (F(0.2), F(0.4), F(0.6), F(0.8))
SATURATED = F(0.9999)   # the march's early-termination bound (oracle/ovr_oracle.c:608-615): a translucent ray ends behind the event that reaches it


MAX_AO_SAMPLES, AO_ROTATIONS = 16, 16
GOLDEN = 0.6180339887498949


def ao_directions(K):
    """the direction table D[m][j] -> (16, K, 3) float32: formed in float64, each component rounded once"""
    K = int(K)
    if K < 0 or K > MAX_AO_SAMPLES:
        raise ValueError("between 0 and 16 ambient-occlusion samples")
    j = np.arange(K, dtype=np.float64)[None, :]
    m = np.arange(AO_ROTATIONS, dtype=np.float64)[:, None]
    r2 = np.broadcast_to((j + 0.5) / K if K else j, (AO_ROTATIONS, K))
    phi = 2.0 * np.pi * (j * GOLDEN + m / 16.0)
    return np.stack([np.sqrt(r2) * np.cos(phi), np.sqrt(r2) * np.sin(phi), np.sqrt(1.0 - r2)], -1).astype(F)


def ao_rotation(x, y, frame_index, spp, k):
    """the table's rotation for sample k of frame frame_index (1-based) at the pixels (x, y): integers only"""
    return ((np.asarray(x, np.int64) & 3) + 4 * (np.asarray(y, np.int64) & 3) + (int(frame_index) - 1) * int(spp) + int(k)) & 15


def ao_facing(n_w, direction):
    """the normal that faces the viewer: n_w where dot(n_w, dir) <= 0, else -n_w (NaN stays NaN)"""
    n_w = np.asarray(n_w, F)
    with np.errstate(invalid="ignore", over="ignore"):
        front = lighting.dot(n_w, np.asarray(direction, F)) <= 0
    return np.where(front[..., None], n_w, -n_w).astype(F)


def ao_basis(N):
    """Duff et al.'s branch-free orthonormal basis around N (n, 3) -> T, B (n, 3), every operation rounding on its own"""
    N = np.asarray(N, F)
    x, y, z = N[..., 0], N[..., 1], N[..., 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.copysign(F(1), z).astype(F)
        a = (F(-1) / (s + z).astype(F)).astype(F)
        b = ((x * y).astype(F) * a).astype(F)
        sx = (s * x).astype(F)
        T = np.stack([(F(1) + ((sx * x).astype(F) * a).astype(F)).astype(F), (s * b).astype(F), -sx], -1)
        B = np.stack([b, (s + ((y * y).astype(F) * a).astype(F)).astype(F), -y], -1)
    return T.astype(F), B.astype(F)


def ao_ray(local, N, T, B):
    """d_c = fma(x, T_c, fma(y, B_c, z N_c)) for the local directions (n, 3)"""
    local = np.asarray(local, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return fma(local[:, 0:1], T, fma(local[:, 1:2], B, (local[:, 2:3] * N).astype(F)))


def isovalues(values):
    """the values as the setter stores them: float32, sorted ascending; ValueError for what it refuses"""
    v = np.sort(np.asarray(values, F).ravel())
    if v.size > MAX_ISOVALUES or not np.isfinite(v).all() or (np.diff(v) == 0).any():
        raise ValueError("at most four finite, distinct isovalues")
    return v


def side(s, iso):
    s = np.asarray(s, F)
    with np.errstate(invalid="ignore"):
        return (np.asarray(iso, F).reshape((1,) * s.ndim + (-1,)) <= s[..., None]).sum(-1)


def product_sampler(volume, vertex_centred=False):
    """the product build's tap of an 8-bit volume: the filter over the stored integers, normalised once behind it; None for the other types (projection.sample)"""
    v = np.asarray(volume)
    if v.dtype == np.uint8:
        raw, scale = v.astype(F), F(1) / F(255)
    elif v.dtype == np.int8:
        raw, scale = np.maximum(v.astype(F), F(-127)), F(1) / F(127)
    else:
        return None
    return lambda po: (sample(raw, po, vertex_centred) * scale).astype(F)


def skipped_side(lo, hi, iso):
    """(fetch, side of a dropped step) from the value ranges of the steps' cells"""
    lo, hi, iso = np.asarray(lo, F), np.asarray(hi, F), np.asarray(iso, F)
    sl = slack(lo, hi)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = (lo - sl).astype(F)[..., None], (hi + sl).astype(F)[..., None]
        below, above = iso < a, iso > b
    return ~(below | above).all(-1), below.sum(-1)


def opacities_of(opacities, iso_as_given):
    """the opacities as the setter stores them: float32, travelling with their isovalues into ascending order; ValueError for what it refuses"""
    v = np.asarray(iso_as_given, F).ravel()
    a = np.asarray(opacities, F).ravel()
    if a.size != v.size or not np.isfinite(a).all() or (a <= 0).any() or (a > 1).any():
        raise ValueError("one opacity in (0, 1] per isovalue")
    return a[np.argsort(v, kind="stable")]


def events_of_step(before, at):
    """the isovalues a step crosses, in the order the ray meets them: rising from side a to b > a: a ... b - 1; falling to b < a: a - 1 ... b"""
    return range(before, at) if at > before else range(before - 1, at - 1, -1)


def walk_events(sd, fetch, count, alpha):
    """the translucent walk over the sides sd (n, width) of the steps: every crossing composited front to back until A >= 0.9999f or the ray's last step.
    -> dict(hit, i, k - the first event's -, walked, fetched, events: per ray a list of (step, k, A after the event))"""
    n, width = sd.shape
    one = F(1)
    hit, first_i, first_k, walked, events = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64), np.asarray(count, np.int64).copy(), []
    for r in range(n):
        ev, A, done = [], F(0), False
        row, c = sd[r], int(count[r])
        for i in (np.flatnonzero(row[1:c] != row[:c - 1]) + 1 if c > 1 else ()):
            for k in events_of_step(int(row[i - 1]), int(row[i])):
                A = F(fma(F(one - A), alpha[k], A))
                ev.append((int(i), int(k), A))
                if A >= SATURATED:
                    done = True
                    break
            if done:
                walked[r] = i + 1
                break
        if ev:
            hit[r], first_i[r], first_k[r] = True, ev[0][0], ev[0][1]
        events.append(ev)
    fetched = (fetch & (np.arange(width)[None, :] < walked[:, None])).sum(1)
    return dict(hit=hit, i=first_i, k=first_k, walked=walked, fetched=fetched, events=events)


def walk(s, count, iso, ranges=None, opacities=None):
    """s (n, width) samples, count (n,) -> dict(hit, i - the hit's step -, k - k* -, walked, fetched): the first crossing.  ranges = (lo, hi), each (n, width): the
    skipping walk, which never looks at a dropped step's sample.  opacities (one per isovalue, ascending with them): the translucent walk (walk_events)"""
    s = np.asarray(s, F)
    n, width = s.shape
    count = np.asarray(count, np.int64)
    sd = side(s, iso)
    fetch = np.ones((n, width), bool)
    if ranges is not None:
        fetch, below = skipped_side(ranges[0], ranges[1], iso)
        sd = np.where(fetch, sd, below)
    if opacities is not None:
        return walk_events(sd, fetch, count, np.asarray(opacities, F))
    idx = np.arange(width)[None, :]
    cross = np.zeros((n, width), bool)
    if width > 1:
        cross[:, 1:] = (sd[:, 1:] != sd[:, :-1]) & (idx[:, 1:] < count[:, None])
    hit = cross.any(1)
    i = np.where(hit, cross.argmax(1), 0)
    r = np.arange(n)
    before, at = sd[r, np.maximum(i - 1, 0)], sd[r, i]
    k = np.where(at > before, before, before - 1)
    walked = np.where(hit, i + 1, count)
    fetched = (fetch & (idx < walked[:, None])).sum(1)
    return dict(hit=hit, i=i, k=np.where(hit, k, 0), walked=walked, fetched=fetched)


def refine(tap, iso, ta, sa, tb, sb):
    """two rounds of four points, then the secant: tap(t) -> samples at the rays' distances t.  Returns (t*, ta, tb) - the last interval with it"""
    ta, sa, tb, sb, iso = (np.asarray(x, F).copy() for x in (ta, sa, tb, sb, iso))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(2):
            w = (tb - ta).astype(F)
            p = [ta] + [fma(c, w, ta) for c in C] + [tb]
            q = [sa] + [tap(pj) for pj in p[1:5]] + [sb]
            inside = [iso <= x for x in q]
            done = np.zeros(ta.shape, bool)
            nta, nsa, ntb, nsb = ta.copy(), sa.copy(), tb.copy(), sb.copy()
            for j in range(5):
                take = ~done & (inside[j] != inside[j + 1])
                nta, nsa = np.where(take, p[j], nta), np.where(take, q[j], nsa)
                ntb, nsb = np.where(take, p[j + 1], ntb), np.where(take, q[j + 1], nsb)
                done |= take
            ta, sa, tb, sb = nta.astype(F), nsa.astype(F), ntb.astype(F), nsb.astype(F)
        f = ((iso - sa).astype(F) / (sb - sa).astype(F)).astype(F)
        t = fmin(fmax(fma(f, (tb - ta).astype(F), ta), ta), tb)
    return t, ta, tb


def normals(tap_object, po, s, dims, inv_scale, vertex_centred=False):
    """shade_request's forward difference at the object positions po (n, 3) with the samples s there -> n_w (n, 3)"""
    n = np.asarray(dims, np.int64)
    g = (F(1) / (n - 1 if vertex_centred else n).astype(F)).astype(F)
    grad = np.empty(po.shape, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(3):
            d = np.where((po[:, k] + g[k]).astype(F) > F(1), -g[k], g[k]).astype(F)
            pk = po.copy()
            pk[:, k] = (po[:, k] + d).astype(F)
            grad[:, k] = ((tap_object(pk) - s).astype(F) / d).astype(F)
        n_o = (-lighting.normalize(grad)).astype(F)
        return lighting.normalize((n_o * np.asarray(inv_scale, F)[None, :]).astype(F))


def trace_rays(volume, org, direction, rate, iso, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, skipping=False, shadows=True, light=None,
               sampler=None, camera_kind=0, opacities=None, ao=None):
    """world rays org, direction (n, 3) - the direction used as given - -> what ovr_hip_isosurface_floats returns per ray, and the counters' parts:
    dict(hit, iso, t, steps, normal (n, 3), shadow, fetched, pos (n, 3), shadow_steps, shadow_fetched, tm_before, tm_at, k); zeros for a ray without a hit.
    light: the raw vector towards the light (normalised here as the host does); sampler(po) replaces projection.sample (product_sampler);
    camera_kind = camera.ORTHOGRAPHIC: the rays are that camera's primary rays (camera.hits: a ray outside an ignored slab misses; shadow rays are untouched).
    opacities (one per isovalue as given): the translucent walk - the keys above describe the ray's FIRST event (steps, fetched: the whole walk; shadow_steps,
    shadow_fetched: the shadow walks of all events), and A (n,), n_events (n,), events (per ray a list of dict(i - the step -, k, t, normal, shadow, A - after the
    event)) and flat (the events of all rays in order: ray, i, k, iso, alpha, t, pos, normal, shadow, A, tm_before, tm_at) are added.
    ao = (table (16, K, 3) - ao_directions(K) or the host's -, R, rotation (n,) - the table's rotation per ray): ambient occlusion (without opacities: all ones) -
    flat and the events gain O, the ray ao_steps and ao_fetched (the AO walks of all its events)"""
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    if ao is not None and opacities is None:
        opacities = np.ones(np.asarray(iso).size, F)
    alpha = None if opacities is None else opacities_of(opacities, iso)
    iso = isovalues(iso)
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    inv, wp = clipping.volume_constants(dims, spacing, origin, vertex_centred)
    lo, hi = ((0, 0, 0), (1, 1, 1)) if clip is None else clip
    step = F(1) / F(rate)
    tap_object = (lambda po: sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    rng = macrocell_ranges(vol) if skipping else None

    def first_crossing(o, d, tm, count):
        n, width = tm.shape
        with np.errstate(invalid="ignore", over="ignore"):
            po = clipping.to_object(fma(np.nan_to_num(tm)[:, :, None], d[:, None, :], o[:, None, :]).reshape(-1, 3), inv, wp)
        s = tap_object(po).reshape(n, width)
        ranges = None
        if skipping:
            c = tap_cell(tap_coordinates(po, dims, vertex_centred)[0], dims)
            r = rng[c[:, 2], c[:, 1], c[:, 0]].reshape(n, width, 2)
            ranges = (r[..., 0], r[..., 1])
        return s, walk(s, count, iso, ranges, alpha)

    if camera_kind:
        from . import camera
        t0, t1, box = camera.hits(org, direction, inv, wp, lo, hi, camera_kind)
    else:
        t0, t1, box = clipping.world_intervals(org, direction, inv, wp, lo, hi)
    tm, count = steps(t0, t1, step, box)
    n = len(org)
    if tm.shape[1] == 0:
        tm = np.zeros((n, 1), F)
    s, w = first_crossing(org, direction, tm, count)
    if alpha is not None:
        return _trace_layers(org, direction, tm, s, w, box, iso, alpha, tap_object, inv, wp, dims, vertex_centred, lo, hi, step, first_crossing, shadows, light, ao)
    hit, r = w["hit"], np.arange(n)
    i = w["i"]
    ta, tb, sa, sb = tm[r, np.maximum(i - 1, 0)], tm[r, i], s[r, np.maximum(i - 1, 0)], s[r, i]
    isov = iso[np.clip(w["k"], 0, len(iso) - 1)] if len(iso) else np.zeros(n, F)
    out = dict(hit=hit, k=w["k"], iso=np.where(hit, isov, F(0)).astype(F), steps=np.where(box, w["walked"], 0), fetched=np.where(box, w["fetched"], 0),
               t=np.zeros(n, F), normal=np.zeros((n, 3), F), shadow=np.zeros(n, F), pos=np.zeros((n, 3), F), shadow_steps=np.zeros(n, np.int64),
               shadow_fetched=np.zeros(n, np.int64), tm_before=np.where(hit, ta, F(0)).astype(F), tm_at=np.where(hit, tb, F(0)).astype(F))
    h = np.flatnonzero(hit)
    if h.size == 0:
        return out
    oh, dh = org[h], direction[h]

    def tap_ray(t):
        with np.errstate(invalid="ignore", over="ignore"):
            return tap_object(clipping.to_object(fma(t[:, None], dh, oh), inv, wp))

    t, _, _ = refine(tap_ray, isov[h], ta[h], sa[h], tb[h], sb[h])
    with np.errstate(invalid="ignore", over="ignore"):
        pos = fma(t[:, None], dh, oh)
    po = clipping.to_object(pos, inv, wp)
    out["t"][h], out["pos"][h] = t, pos
    out["normal"][h] = normals(tap_object, po, tap_object(po), dims, inv, vertex_centred)
    if shadows:
        L = lighting.normalize(np.asarray(lighting.LITERAL_LIGHT if light is None else light, F))
        Ld = np.broadcast_to(L, pos.shape)
        s0, s1, sbox = clipping.world_intervals(pos, Ld, inv, wp, lo, hi)
        stm, scount = steps((s0 + step).astype(F), s1, step, sbox)
        if stm.shape[1] == 0:
            stm = np.zeros((h.size, 1), F)
        _, sw = first_crossing(pos, Ld, stm, scount)
        out["shadow"][h] = sw["hit"].astype(F)
        out["shadow_steps"][h] = np.where(sbox, sw["walked"], 0)
        out["shadow_fetched"][h] = np.where(sbox, sw["fetched"], 0)
    return out


def _trace_layers(org, direction, tm, s, w, box, iso, alpha, tap_object, inv, wp, dims, vertex_centred, lo, hi, step, first_crossing, shadows, light, ao=None):
    """trace_rays behind the translucent walk w: every event refined, shaded and shadowed as the opaque hit is"""
    n = len(org)
    ev = [(r, i, k, A) for r, row in enumerate(w["events"]) for (i, k, A) in row]
    er, ei, ek = (np.array([e[j] for e in ev], np.int64) for j in range(3))
    eA = np.array([e[3] for e in ev], F)
    m = len(ev)
    n_events = np.array([len(row) for row in w["events"]], np.int64)
    flat = dict(ray=er, i=ei, k=ek, iso=iso[ek] if m else np.zeros(0, F), alpha=alpha[ek] if m else np.zeros(0, F), t=np.zeros(m, F), pos=np.zeros((m, 3), F),
                normal=np.zeros((m, 3), F), shadow=np.zeros(m, F), A=eA, tm_before=tm[er, ei - 1] if m else np.zeros(0, F), tm_at=tm[er, ei] if m else np.zeros(0, F))
    shadow_steps, shadow_fetched = np.zeros(m, np.int64), np.zeros(m, np.int64)
    if m:
        oh, dh = org[er], direction[er]

        def tap_ray(t):
            with np.errstate(invalid="ignore", over="ignore"):
                return tap_object(clipping.to_object(fma(t[:, None], dh, oh), inv, wp))

        t, _, _ = refine(tap_ray, flat["iso"], tm[er, ei - 1], s[er, ei - 1], tm[er, ei], s[er, ei])
        with np.errstate(invalid="ignore", over="ignore"):
            pos = fma(t[:, None], dh, oh)
        po = clipping.to_object(pos, inv, wp)
        flat["t"], flat["pos"] = t, pos
        flat["normal"] = normals(tap_object, po, tap_object(po), dims, inv, vertex_centred)
        if shadows:
            L = lighting.normalize(np.asarray(lighting.LITERAL_LIGHT if light is None else light, F))
            Ld = np.broadcast_to(L, pos.shape)
            s0, s1, sbox = clipping.world_intervals(pos, Ld, inv, wp, lo, hi)
            stm, scount = steps((s0 + step).astype(F), s1, step, sbox)
            if stm.shape[1] == 0:
                stm = np.zeros((m, 1), F)
            _, sw = first_crossing(pos, Ld, stm, scount)
            flat["shadow"] = np.array([row[-1][2] if row else F(0) for row in sw["events"]], F)
            shadow_steps, shadow_fetched = np.where(sbox, sw["walked"], 0), np.where(sbox, sw["fetched"], 0)
    ao_steps, ao_fetched = np.zeros(m, np.int64), np.zeros(m, np.int64)
    if ao is not None:
        flat["O"] = np.zeros(m, F)
    if m and ao is not None:
        table, R, rot = np.asarray(ao[0], F), F(ao[1]), np.asarray(ao[2], np.int64).ravel()
        K = table.shape[1]
        N = ao_facing(flat["normal"], dh)
        T, B = ao_basis(N)
        local = table[rot[er] & 15]   # (m, K, 3)
        S = np.zeros(m, F)
        for j in range(K):
            d = ao_ray(local[:, j], N, T, B)
            a0, a1, abox = clipping.world_intervals(pos, d, inv, wp, lo, hi)
            atm, acount = steps((a0 + step).astype(F), fmin(a1, R), step, abox)
            if atm.shape[1] == 0:
                atm = np.zeros((m, 1), F)
            _, aw = first_crossing(pos, np.where(abox[:, None], d, F(0)).astype(F), atm, acount)   # (a ray that misses the box has no step: its direction is not read)
            S = (S + np.array([row[-1][2] if row else F(0) for row in aw["events"]], F)).astype(F)
            ao_steps += np.where(abox, aw["walked"], 0)
            ao_fetched += np.where(abox, aw["fetched"], 0)
        flat["O"] = (S / F(K)).astype(F)
    first = np.concatenate([[0], np.cumsum(n_events)[:-1]]).astype(np.int64)   # a ray's first event in the flat order
    hit = n_events > 0
    f = first[hit]
    out = dict(hit=hit, k=w["k"], iso=np.zeros(n, F), steps=np.where(box, w["walked"], 0), fetched=np.where(box, w["fetched"], 0), t=np.zeros(n, F),
               normal=np.zeros((n, 3), F), shadow=np.zeros(n, F), pos=np.zeros((n, 3), F), shadow_steps=np.zeros(n, np.int64), shadow_fetched=np.zeros(n, np.int64),
               tm_before=np.zeros(n, F), tm_at=np.zeros(n, F), A=np.zeros(n, F), n_events=n_events, flat=flat)
    for key in ("iso", "t", "normal", "shadow", "pos"):
        out[key][hit] = flat[key][f]
    out["tm_before"][hit], out["tm_at"][hit] = tm[er[f], ei[f] - 1], tm[er[f], ei[f]]
    np.add.at(out["shadow_steps"], er, shadow_steps)
    np.add.at(out["shadow_fetched"], er, shadow_fetched)
    if ao is not None:
        out["ao_steps"], out["ao_fetched"] = np.zeros(n, np.int64), np.zeros(n, np.int64)
        np.add.at(out["ao_steps"], er, ao_steps)
        np.add.at(out["ao_fetched"], er, ao_fetched)
    last = first + n_events - 1
    out["A"][hit] = eA[last[hit]]
    out["events"] = [[dict(i=int(ei[j]), k=int(ek[j]), t=flat["t"][j], normal=flat["normal"][j], shadow=flat["shadow"][j], A=eA[j], **({} if ao is None else dict(O=flat["O"][j])))
                      for j in range(first[r], first[r] + n_events[r])] for r in range(n)]
    return out


def composite(flat, rgb, n):
    """the events' colours rgb (m, 3) composited per ray front to back by the march's recurrence -> C (n, 3) premultiplied, A (n,)"""
    Cc, A = np.zeros((n, 3), F), np.zeros(n, F)
    ray, alpha = flat["ray"], flat["alpha"]
    if len(ray) == 0:
        return Cc, A
    ordinal = np.arange(len(ray)) - np.searchsorted(ray, ray, side="left")   # (the flat order is by ray, then along the ray)
    for e in range(int(ordinal.max()) + 1):
        j = np.flatnonzero(ordinal == e)
        r = ray[j]
        tr = (F(1) - A[r]).astype(F)
        Cc[r] = fma((tr[:, None] * rgb[j]).astype(F), alpha[j][:, None], Cc[r])
        A[r] = fma(tr, alpha[j], A[r])
    return Cc, A


def frame(volume, basis, size, rate, iso, colors, tf_range, shading=FULL, light=None, intensity=1.0, material=lighting.REFERENCE_MATERIAL, spacing=(1, 1, 1),
          origin=(0, 0, 0), vertex_centred=False, clip=None, skipping=False, spp=1, noise=None, frame_index=1, sampler=None, camera_kind=0, opacities=None, ao=None):
    """one isosurface frame: rgba (H, W, 4), layer (H, W, 3) and counters (opacities: the translucent frame - `hits` counts the events composited).  basis = (pos, dir, hor, ver); tf_range in the samples' units
    (projection.normalized_range); noise = the blue-noise tile switches that jitter on - without it spp must be 1, as in projection.frame;
    camera_kind = camera.ORTHOGRAPHIC: the basis is an orthographic camera's - rays from camera.pixel_rays, the view vector -dir (the default: today's frame);
    ao = (table (16, K, 3), R): ambient occlusion under GRADIENT / FULL (K = 0 or NONE: not cast) - the counters' ao_steps / ao_fetched are its walks' steps"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, active_pixels=h * w, steps=0, fetched=0, hits=0, shadow_steps=0, shadow_fetched=0, ao_steps=0, ao_fetched=0)
    if ao is not None and (shading == NONE or np.asarray(ao[0]).shape[1] == 0):
        ao = None
    if ao is not None and opacities is None:
        opacities = np.ones(np.asarray(iso).size, F)   # the opaque frame through the translucent text
    py, px = np.mgrid[0:h, 0:w]
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    raw_light = lighting.LITERAL_LIGHT if light is None else light
    L = lighting.normalize(np.asarray(raw_light, F))
    ka, kd, ks, shin = material
    for k in range(spp):
        xi = None if noise is None else blue_noise_variates(noise, w, h, frame_index, spp, k)
        d = pixel_rays(basis, w, h, xi).reshape(-1, 3)
        view = None
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
            view = camera.view_vector(basis) if camera_kind == camera.ORTHOGRAPHIC else None
        rays_ao = None if ao is None else (ao[0], ao[1], ao_rotation(px, py, frame_index, spp, k).ravel())
        r = trace_rays(volume, org, d, rate, iso, spacing, origin, vertex_centred, clip, skipping, shading == FULL, raw_light, sampler, camera_kind, opacities, rays_ao)
        m = r["hit"]
        e = r if opacities is None else r["flat"]   # what is coloured and shaded: the hit, or every event
        rgb = classify(e["iso"], colors, np.zeros(2, F), *tf_range)[:, :3]
        if shading != NONE:
            amb = ka if ao is None else (F(ka) * (F(1) - e["O"]).astype(F)).astype(F)
            f = lighting.shade(e["normal"], e["pos"], e["shadow"], L, basis[0], amb, kd, ks, shin, intensity, view=view)
            with np.errstate(invalid="ignore", over="ignore"):
                rgb = clamp01((rgb * f[:, None]).astype(F))
        if opacities is None:
            c = np.concatenate([rgb, np.ones((h * w, 1), F)], 1)
        else:   # un-premultiplied, like the march's pixel
            Cc, A = composite(e, rgb, h * w)
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.concatenate([(Cc / A[:, None]).astype(F), A[:, None]], 1)
        rgba = (rgba + np.where(m[:, None], c, F(0))).astype(F)
        layer = (layer + np.where(m[:, None], np.stack([r["iso"], r["t"], np.ones(h * w, F)], 1), F(0))).astype(F)
        counters["rays"] += h * w
        counters["steps"] += int(r["steps"].sum())
        counters["fetched"] += int(r["fetched"].sum())
        counters["hits"] += int(m.sum()) if opacities is None else len(e["ray"])
        counters["shadow_steps"] += int(r["shadow_steps"].sum())
        counters["shadow_fetched"] += int(r["shadow_fetched"].sum())
        if ao is not None:
            counters["ao_steps"] += int(r["ao_steps"].sum())
            counters["ao_fetched"] += int(r["ao_fetched"].sum())
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
