"""Pre-integrated classification of the HIP backend (include/ovr_hip.h, ovr_hip_set_preintegration) as a numpy model: the normative text.

The unshaded march classifies a sample point by point: one tap at the middle of a step, one lookup in the 1-D transfer function, the opacity correction.  A
pre-integrated frame classifies the SEGMENT between two consecutive samples by the integral of the transfer function over the values the segment spans
(Engel et al. 2001), read from a node table of cumulative integrals.  The ray, the box test and the tap are clipping.py's and projection.py's, the
deterministic log2 / exp2 pair lighting.py's, the opacity correction slice_context.py's: imported here, not restated.

The node table (node_table; host side, float64, rounded ONCE to float32):

    M     = S * max(n_alpha - 1, n_color - 1, 1) + 1 nodes, node j at u_j = j / (M - 1); S is 4, 2 or 1 (subdivision: the largest whose table fits the LDS budget)
    a_j   = clamp01 of the alpha table's nodal lerp at u_j, c_j = clamp01 per channel of the colour table's lerp - in float64 from the float32 entries:
            x = u * (n - 1), i0 = floor(x), the pair (i0, min(i0 + 1, n - 1)), a + (x - i0) * (b - a)
    tau_j = -log2(1 - min(a_j, 1 - 2^-24))
    T_j, K_j (rgb) = the cumulative trapezoid sums of tau and of tau * c over u: T_j = T_(j-1) + 0.5 * (tau_(j-1) + tau_j) * (1 / (M - 1))
    a node is the float32 quadruple (T, Kr, Kg, Kb)

Per pixel sample (world origin o, direction d; t0, t1, hit, step = 1 / rate and base = 1 as in the unshaded march; float32, fma fused, everything else rounds on
its own):

    alpha = 0, C = 0, tx = t0, ty = fmin(t1, t0 + step)
    uf = tf_coord(the tap at to_object(fma(tx, d, o)))                    the entry tap - NOT counted in `samples`
    while ty > tx and alpha < 0.9999:
        ub = tf_coord(the tap at to_object(fma(ty, d, o)))                ONE tap per segment, at its back end
        du = ub - uf;  dt = ty - tx;  adj = base * dt
        if fabs(du) * (M - 1) < 1:                                        less than a node apart: the march's own classification
            um = 0.5 * (uf + ub)
            a  = opacity_correction(tf_alpha(um), adj)                    (with its nearly-equal shortcut)
            c  = clamp01(tf_color(um))
        else:                                                             the integral branch
            (Tf, Kf), (Tb, Kb) = the node lerp at uf, ub                  x = u * (M - 1), i0 = (int)x, f = x - i0, fma(f, n[i0 + 1] - n[i0], n[i0]) per component
            Td = Tb - Tf
            a  = clamp01(1 - det_exp2(-((Td / du) * adj)))
            c  = clamp01((Kb - Kf) / Td) per channel if Td != 0 else 0
        tr = 1 - alpha
        C_ch = fma(tr * c_ch, a, C_ch);  alpha = fma(tr, a, alpha)
        tx = ty;  ty = fmin(tx + step, t1);  uf = ub
    the sample: a = alpha; rgb = C / a per channel if a > 0, else 0 - the march's un-premultiplied pixel
    counters: samples = segments taken; shaded_samples = segments with a > 0; nothing is skipped; the gradient layer is zero

Consequences.  Over a constant volume every tap returns the voxels' value exactly (lerp(a, a, f) = a), every segment takes the first branch with um = uf, and
the frame is the unshaded march's bit for bit, counters included.  Along an axis-parallel ray through a volume that is a linear ramp along that axis du = slope *
dt, so Td / du * dt telescopes: the ray's transmittance is 2^-((T~(u_end) - T~(u_begin)) / slope) whatever the rate (T~: the node lerp), up to rounding and
the first-branch segments in the clamp-to-edge half voxels at the faces."""
import numpy as np

from . import clipping, projection
from .clipping import clamp01, fmax, fmin
from .lighting import det_exp2, fma
from .slice_context import opacity_correction

F = np.float32
OFF, SEGMENTS = 0, 1
ERT = F(0.9999)   # the march's early-termination literal
BASE = F(1)       # the march's `base`
SUBDIVISIONS = (4, 2, 1)
LDS_BUDGET = (160 * 1024 // 3) & ~15   # csrc/host/launch_plan.hpp kPreintegrationLdsBudget: three workgroups per CU


def commit(mode):
    """the mode as ovr_hip_set_preintegration stores it; ValueError where it returns EINVAL"""
    if mode not in (OFF, SEGMENTS):
        raise ValueError("the pre-integration mode is OFF or SEGMENTS")
    return int(mode)


def active(mode, shading=0, slices=0, isovalues=0, projection_mode=0):
    """a frame is pre-integrated iff the committed frame is the march, the committed shading mode is NONE and the mode is SEGMENTS"""
    return commit(mode) == SEGMENTS and shading == 0 and not slices and not isovalues and not projection_mode


def node_count(n_color, n_alpha, subdivision):
    return int(subdivision) * max(int(n_alpha) - 1, int(n_color) - 1, 1) + 1


def subdivision(n_color, n_alpha, room):
    """the largest of 4, 2, 1 whose table of 16 * (M + 1) bytes fits in `room` bytes of LDS; 0: none does"""
    for s in SUBDIVISIONS:
        if 16 * (node_count(n_color, n_alpha, s) + 1) <= room:
            return s
    return 0


def _table_lerp64(table, u):
    """the nodal lerp of a float32 table (n,) or (n, k) at u (float64), in float64"""
    t = np.asarray(table, F).astype(np.float64)
    n1 = len(t) - 1
    x = u * float(n1)
    i0 = np.minimum(np.floor(x).astype(np.int64), n1)
    i1 = np.minimum(i0 + 1, n1)
    f = x - i0
    if t.ndim == 2:
        f = f[:, None]
    return t[i0] + f * (t[i1] - t[i0])


def _clamp01_64(x):
    return np.where(x == x, np.minimum(np.maximum(x, 0.0), 1.0), 0.0)


def node_table(colors, alphas, subdivision=4):
    """the float32 node table (M, 4) - T, Kr, Kg, Kb - of the tables as committed: colours (Nc, 3), alphas (Na,)"""
    colors, alphas = np.asarray(colors, F).reshape(-1, 3), np.asarray(alphas, F).ravel()
    m = node_count(len(colors), len(alphas), subdivision)
    h = 1.0 / float(m - 1)
    u = np.arange(m, dtype=np.float64) / float(m - 1)
    a = _clamp01_64(_table_lerp64(alphas, u))
    c = _clamp01_64(_table_lerp64(colors, u))
    tau = -np.log2(1.0 - np.minimum(a, 1.0 - 2.0 ** -24))
    kc = tau[:, None] * c
    # the sums start from +0 and add node by node (a transparent stretch stays +0: tau = -log2(1) is -0)
    steps = np.concatenate([np.zeros((1, 4)), np.concatenate([(0.5 * (tau[:-1] + tau[1:]) * h)[:, None], 0.5 * (kc[:-1] + kc[1:]) * h], 1)], 0)
    return np.cumsum(steps, axis=0).astype(F)


def tf_coord(v, lower, upper):
    """projection.classify's coordinate: clamp01((clamp(v, lower, upper) - lower) * scale), scale = 0 for a degenerate range"""
    v = np.asarray(v, F).ravel()
    lower, upper = F(lower), F(upper)
    scale = F(0) if upper == lower else F(1) / F(upper - lower)
    with np.errstate(invalid="ignore", over="ignore"):
        return clamp01(((fmin(fmax(v, lower), upper) - lower).astype(F) * scale).astype(F))


def table_lookup(table, u):
    """projection.classify's nodal lerp of a committed table (n,) or (n, k) at the coordinate u (float32)"""
    table = np.asarray(table, F)
    if table.ndim == 1:
        table = table[:, None]
    n1 = len(table) - 1
    x = (np.asarray(u, F) * F(n1)).astype(F)
    i0 = x.astype(np.int64)
    f = (x - np.floor(x)).astype(F)
    i1 = np.minimum(i0 + 1, n1)
    return np.stack([projection.lerp(table[i0, k], table[i1, k], f) for k in range(table.shape[1])], 1)


def node_lerp(nodes, u):
    """(T, Kr, Kg, Kb) (n, 4) float32 at the coordinates u: x = u * (M - 1), i0 = (int)x, its fraction, the lerp of nodes i0 and i0 + 1 (a copy of the last)"""
    return table_lookup(np.asarray(nodes, F).reshape(-1, 4), u)


def preintegrated_rays(volume, org, direction, rate, colors, alphas, tf_range, nodes=None, subdivision=4, spacing=(1, 1, 1), origin=(0, 0, 0),
                       vertex_centred=False, clip=None, sampler=None, camera_kind=0, border=1e-5, du_border=1e-4):
    """world rays org, direction (n, 3) - the direction used as given: dict(steps (segments taken), integral (of them on the integral branch), tx (at exit; 0 for
    a ray that is not hit), rgba (n, 4) of the sample, shaded (segments with a > 0), rays_hit, and - for comparisons with a build whose exp2 / pow differ in
    their last bit - borderline (a loop test met an alpha within `border` of 0.9999), hinge (the segments from t0 to t1 of such a ray: what its count may
    differ by), branch_borderline (a segment whose fabs(du) * (M - 1) lies within du_border of 1: which branch it takes rests on the tap's last bits)).
    nodes: the float32 node table (M, 4) the frames read - the library's own in the GPU tests -, else node_table(colors, alphas, subdivision)"""
    vol = np.asarray(volume)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    org, direction = np.asarray(org, F).reshape(-1, 3), np.asarray(direction, F).reshape(-1, 3)
    nodes = node_table(colors, alphas, subdivision) if nodes is None else np.asarray(nodes, F).reshape(-1, 4)
    fm1 = F(len(nodes) - 1)
    inv, wp = clipping.volume_constants(dims, spacing, origin, vertex_centred)
    lo, hi = ((0, 0, 0), (1, 1, 1)) if clip is None else clip
    if camera_kind:
        from . import camera
        t0, t1, hit = camera.hits(org, direction, inv, wp, lo, hi, camera_kind)
    else:
        t0, t1, hit = clipping.world_intervals(org, direction, inv, wp, lo, hi)
    m = len(t0)
    tap = (lambda po: projection.sample(vol, po, vertex_centred)) if sampler is None else (lambda po: np.asarray(sampler(po), F))
    coord = lambda t, idx: tf_coord(tap(clipping.to_object(fma(t[:, None], direction[idx], org[idx]), inv, wp)), *tf_range)
    step = F(1) / F(rate)
    alpha, C = np.zeros(m, F), np.zeros((m, 3), F)
    steps, integral, shaded = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    near, near_branch = np.zeros(m, bool), np.zeros(m, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tx = t0.copy()
        ty = fmin(t1, (t0 + step).astype(F))
        live = hit.copy()
        uf = np.zeros(m, F)
        idx = np.flatnonzero(live)
        if idx.size:
            uf[idx] = coord(tx[idx], idx)
        while True:
            near |= live & (ty > tx) & (np.abs(alpha.astype(np.float64) - float(ERT)) <= border)
            live = live & (ty > tx) & (alpha < ERT)
            idx = np.flatnonzero(live)
            if not idx.size:
                break
            x, y, f_ = tx[idx], ty[idx], uf[idx]
            ub = coord(y, idx)
            du = (ub - f_).astype(F)
            adj = (BASE * (y - x).astype(F)).astype(F)
            spread = (np.abs(du) * fm1).astype(F)
            first = spread < F(1)
            near_branch[idx] |= np.abs(spread.astype(np.float64) - 1.0) <= du_border
            um = (F(0.5) * (f_ + ub).astype(F)).astype(F)
            a1 = opacity_correction(table_lookup(alphas, um)[:, 0], BASE, (y - x).astype(F))
            c1 = clamp01(table_lookup(colors, um))
            nf, nb = node_lerp(nodes, f_), node_lerp(nodes, ub)
            td = (nb[:, 0] - nf[:, 0]).astype(F)
            a2 = clamp01((F(1) - det_exp2((-(((td / du).astype(F) * adj).astype(F))).astype(F))).astype(F))
            some = td != 0
            c2 = np.where(some[:, None], clamp01(((nb[:, 1:] - nf[:, 1:]).astype(F) / np.where(some, td, F(1))[:, None]).astype(F)), F(0)).astype(F)
            a = np.where(first, a1, a2).astype(F)
            c = np.where(first[:, None], c1, c2).astype(F)
            tr = (F(1) - alpha[idx]).astype(F)
            C[idx] = fma((tr[:, None] * c).astype(F), a[:, None], C[idx])
            alpha[idx] = fma(tr, a, alpha[idx])
            steps[idx] += 1
            integral[idx] += ~first
            shaded[idx] += a > 0
            uf[idx] = ub
            tx = np.where(live, ty, tx).astype(F)
            ty = np.where(live, fmin((tx + step).astype(F), t1), ty).astype(F)
    _, whole = projection.steps(t0, t1, step, hit)
    rgba = np.zeros((m, 4), F)
    pos = alpha > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rgba[:, :3] = np.where(pos[:, None], (C / np.where(pos, alpha, F(1))[:, None]).astype(F), F(0))
    rgba[:, 3] = alpha
    return dict(steps=steps, integral=integral, tx=np.where(hit, tx, F(0)).astype(F), rgba=rgba, shaded=shaded, rays_hit=hit, borderline=near,
                hinge=np.where(near, whole, 0), branch_borderline=near_branch)


def frame(volume, basis, size, rate, colors, alphas, tf_range, nodes=None, subdivision=4, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None,
          sampler=None, spp=1, noise=None, frame_index=1, camera_kind=0):
    """one pre-integrated frame: rgba (H, W, 4) and counters (rays, active_pixels, samples, shaded, integral; hinge and the borderline pixel masks, see
    preintegrated_rays).  The arguments are slice_context.frame's without the slices"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    rgba = np.zeros((h * w, 4), F)
    counters = dict(rays=0, active_pixels=h * w, samples=0, shaded=0, integral=0, hinge=0)
    borderline, branch = np.zeros(h * w, bool), np.zeros(h * w, bool)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    for j in range(spp):
        xi = None if noise is None else projection.blue_noise_variates(noise, w, h, frame_index, spp, j)
        d = projection.pixel_rays(basis, w, h, xi).reshape(-1, 3)
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
        r = preintegrated_rays(volume, org, d, rate, colors, alphas, tf_range, nodes, subdivision, spacing, origin, vertex_centred, clip, sampler, camera_kind)
        rgba = (rgba + r["rgba"]).astype(F)
        counters["rays"] += h * w
        counters["samples"] += int(r["steps"].sum())
        counters["shaded"] += int(r["shaded"].sum())
        counters["integral"] += int(r["integral"].sum())
        counters["hinge"] += int(r["hinge"].sum())
        borderline |= r["borderline"]
        branch |= r["branch_borderline"]
    counters["borderline"], counters["branch_borderline"] = borderline.reshape(h, w), branch.reshape(h, w)
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), counters
