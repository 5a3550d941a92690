"""The projections of the HIP backend (include/ovr_hip.h, ovr_hip_set_projection) as a numpy model: the normative text.

A projection is the unshaded march without its sequential part: per ray the MAXIMUM, the MINIMUM or the MEAN of the samples the
march would classify, and ONE classification of that value.  Everything is float32; fma is a fused multiply-add, every other
operation rounds on its own (the kernels are built with -ffp-contract=off).

The ray (`pixel_rays`): exactly the march's for the pixel sample.  With the camera basis (pos, dir, hor, ver) of the host,

    sx = (ix + .5) * (1 / W) [+ (xi0 - .5) * (1 / W)],  sy likewise        xi: the blue-noise variates of the sample, if that jitter is on
    d  = normalize_exact(dir + (sx - .5) * hor + (sy - .5) * ver)         l = sqrt(fma(x, x, fma(y, y, z * z))), d = v / l
    oo = fma(pos, inv_scale, wto_p),  od = d * inv_scale                  the object-space ray: t is shared with world space
    (t0, t1, hit) = clipping.intersect(oo, od, lo, hi) from (0, FLT_MAX)  the clipped test while a clip box is committed

A ray is marched iff hit.

Steps (`steps`): tx_0 = t0, ty_0 = fmin(t1, t0 + step); step i exists while ty_i > tx_i; tm_i = 0.5 * (tx_i + ty_i);
tx_{i+1} = ty_i, ty_{i+1} = fmin(tx_{i+1} + step, t1); n = the number of steps; step = 1 / sampling rate.
The sample s_i is the trilinear tap (`sample`) at to_object(fma(tm_i, d, pos)) - the same tap, the same units as the march
classifies, for every voxel type and grid convention.

Modes (`reduce`):
    MAXIMUM  (m, tm*) = (-inf, 0); in step order: if s_i > m: m = s_i, tm* = tm_i.  v = m.  A NaN is never selected; of equal
             samples the first gives tm* and the bits of v.
    MINIMUM  the same from +inf with s_i < m.
    MEAN     A[0..3] = +0; in step order A[i & 3] = A[i & 3] + s_i; v = ((A0 + A1) + (A2 + A3)) / float32(n); tm* = 0.
             (four interleaved sums: what four lanes per ray compute)

The pixel sample (`classify`): not marched or n == 0: rgba = 0, layer = 0.  Otherwise with c = clamp01((fmin(fmax(v, lower),
upper) - lower) * scale) rgb = clamp01 of the colour table's nodal lerp at c * (Nc - 1) and a = the alpha table's at c * (Na - 1),
no opacity correction; the layer is (v, tm*, 1).  The samples of a pixel are summed in order and multiplied by 1 / spp.

Range skipping (`slack`, `tap_cell`, `reduce_skipping`): the fetch of a step may be dropped when the value range [lo_c, hi_c] of the
macrocell that holds its tap proves that it cannot change (v, tm*).  The filter rounds - fma(f, b - a, a) can land beyond
max(a, b) - so the proof carries a slack, derived from the tap's arithmetic:

    every sample of a tap in cell c lies in [lo_c - S, hi_c + S],   S = fma(2^-21, (hi_c - lo_c) + max(|lo_c|, |hi_c|), FLT_MIN)

Each of the three lerp levels is off by at most u (W + M) (1 + O(u)) with u = 2^-24, W the range's width and M its magnitude (one
rounding of b - a scaled by f <= 1, one of the fma); the 8-bit types, which the product normalises once behind the filter, add
3 u M; forming the bound rounds once more: < 7 u (W + M), taken as 8 u = 2^-21 so that the product is exact.  FLT_MIN covers
gradual underflow (six roundings of at most 2^-150 each).  A step of MAXIMUM is skipped iff hi_c + S <= B, of MINIMUM iff
lo_c - S >= B, where B is the ray's extremum over the ROUNDS (16 steps) before the step's own: every step B comes from is earlier
than the skipped one, so an equal sample would not have replaced it, and `<=` is exact.  MEAN fetches every step."""
import numpy as np

from . import clipping
from .clipping import FLT_MAX, FLT_MIN, clamp01, fmax, fmin
from .lighting import fma

F = np.float32
OFF, MAXIMUM, MINIMUM, MEAN = 0, 1, 2, 3
ROUND = 16  # steps per round of the kernels: four lanes x four instructions


# ---- the ray ---------------------------------------------------------------------------------------------------------------------------
def camera_basis(eye, at, up, fovy, width, height):
    """(pos, dir, hor, ver) as the host derives them (float32; the tangent is libm's tanf there - tests pass the basis the oracle returns)"""
    eye, at, up = (np.asarray(v, F) for v in (eye, at, up))

    def norm(v):
        l = np.sqrt(fma(v[0], v[0], fma(v[1], v[1], F(v[2] * v[2]))))
        return ((v * F(1)) / l).astype(F)

    def cross(a, b):
        return np.array([F(a[1] * b[2]) - F(b[1] * a[2]), F(a[2] * b[0]) - F(b[2] * a[0]), F(a[0] * b[1]) - F(b[0] * a[1])], F)

    t = F(2) * F(np.tan(F(F(F(fovy) * F(0.5)) * F(np.pi)) / F(180)))
    aspect = F(width) / F(height)
    d = norm((at - eye).astype(F))
    hor = (F(t * aspect) * norm(cross(d, up))).astype(F)
    ver = (cross(hor, d) / aspect).astype(F)
    return eye, d, hor, ver


def normalize_exact(v):
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.sqrt(fma(v[..., 0], v[..., 0], fma(v[..., 1], v[..., 1], (v[..., 2] * v[..., 2]).astype(F)))).astype(F)
        return (v / l[..., None]).astype(F)


def pixel_rays(basis, width, height, xi=None):
    """world directions (H, W, 3) of the pixel samples; xi = (xi0, xi1), each (H, W): the jitter variates of the sample, None = the pixel centre"""
    pos, d, hor, ver = (np.asarray(v, F) for v in basis)
    rsx, rsy = F(1) / F(width), F(1) / F(height)
    sx = ((np.arange(width, dtype=F) + F(0.5)) * rsx).astype(F)[None, :].repeat(height, 0)
    sy = ((np.arange(height, dtype=F) + F(0.5)) * rsy).astype(F)[:, None].repeat(width, 1)
    if xi is not None:
        sx = (sx + ((np.asarray(xi[0], F) - F(0.5)).astype(F) * rsx).astype(F)).astype(F)
        sy = (sy + ((np.asarray(xi[1], F) - F(0.5)).astype(F) * rsy).astype(F)).astype(F)
    ux, uy = (sx - F(0.5)).astype(F), (sy - F(0.5)).astype(F)
    v = np.empty((height, width, 3), F)
    for k in range(3):
        v[..., k] = ((d[k] + (ux * hor[k]).astype(F)).astype(F) + (uy * ver[k]).astype(F)).astype(F)
    return normalize_exact(v)


def blue_noise_variates(tile, width, height, frame_index, spp, k):
    """(xi0, xi1), each (H, W), of sample k of frame `frame_index` (1-based): tile in the layout set_noise_tile takes, [y][x][t] with 64 slices"""
    tile = np.asarray(tile, F)
    xy = int(round((tile.size // 64) ** 0.5))
    tile = tile.reshape(xy, xy, 64)
    t = ((int(frame_index) - 1) * int(spp) + int(k)) % 64
    h = xy >> 1
    iy, ix = np.mgrid[0:height, 0:width]
    return tile[iy % xy, ix % xy, t], tile[(iy + h) % xy, (ix + h) % xy, t]


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def steps(t0, t1, step, marched=None):
    """t0, t1 (n,), step: a float32 scalar -> (tm (n, max_steps) float32 - padded with NaN -, count (n,)); rays with marched == False have no step"""
    t0, t1 = np.asarray(t0, F).ravel(), np.asarray(t1, F).ravel()
    step = F(step)
    live = np.ones(t0.shape, bool) if marched is None else np.asarray(marched, bool).ravel().copy()
    with np.errstate(invalid="ignore", over="ignore"):
        tx = t0.copy()
        ty = fmin(t1, (t0 + step).astype(F))
        cols, count = [], np.zeros(t0.shape, np.int64)
        while True:
            live = live & (ty > tx)
            if not live.any():
                break
            cols.append(np.where(live, (F(0.5) * (tx + ty).astype(F)).astype(F), F(np.nan)))
            count += live
            tx = ty
            ty = fmin((tx + step).astype(F), t1)
    tm = np.stack(cols, 1) if cols else np.zeros((t0.size, 0), F)
    return tm.astype(F), count


# ---- the tap ---------------------------------------------------------------------------------------------------------------------------
def voxel_values(volume):
    """the (nz, ny, nx) array as float32 in the units the march classifies: 8-bit types normalised voxel by voxel (v / 255, max(v / 127, -1)), 16-bit types
    raw, 32-bit integers normalised, float64 rounded"""
    v = np.asarray(volume)
    if v.dtype == np.uint8:
        return (v.astype(F) / F(255)).astype(F)
    if v.dtype == np.int8:
        return np.maximum((v.astype(F) / F(127)).astype(F), F(-1))
    if v.dtype == np.uint32:
        return (v.astype(F) / F(0xffffffff)).astype(F)
    if v.dtype == np.int32:
        return np.maximum((v.astype(F) / F(0x7fffffff)).astype(F), F(-1))
    return v.astype(F)


def tap_coordinates(po, dims, vertex_centred=False):
    """object positions (n, 3) -> (i0 (n, 3) int64 in [-1, n - 1], f (n, 3) float32): floor and fraction of x = fma(clamp01(p), cs, cb)"""
    po = np.asarray(po, F).reshape(-1, 3)
    n = np.asarray(dims, np.int64)
    cs = (n - 1 if vertex_centred else n).astype(F)
    cb = np.full(3, 0.0 if vertex_centred else -0.5, F)
    x = fma(clamp01(po), cs[None, :], cb[None, :])
    fl = np.floor(x)
    return fl.astype(np.int64), (x - fl).astype(F)


def lerp(a, b, f):
    with np.errstate(invalid="ignore", over="ignore"):
        return fma(f, (np.asarray(b, F) - np.asarray(a, F)).astype(F), a)


def sample(volume, po, vertex_centred=False):
    """the trilinear tap with clamp-to-edge texels at object positions po (n, 3): lerps along x, then y, then z"""
    v = voxel_values(volume)
    nz, ny, nx = v.shape
    i0, f = tap_coordinates(po, (nx, ny, nz), vertex_centred)
    x0, x1 = np.clip(i0[:, 0], 0, nx - 1), np.clip(i0[:, 0] + 1, 0, nx - 1)
    y0, y1 = np.clip(i0[:, 1], 0, ny - 1), np.clip(i0[:, 1] + 1, 0, ny - 1)
    z0, z1 = np.clip(i0[:, 2], 0, nz - 1), np.clip(i0[:, 2] + 1, 0, nz - 1)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    c00, c10 = lerp(v[z0, y0, x0], v[z0, y0, x1], fx), lerp(v[z0, y1, x0], v[z0, y1, x1], fx)
    c01, c11 = lerp(v[z1, y0, x0], v[z1, y0, x1], fx), lerp(v[z1, y1, x0], v[z1, y1, x1], fx)
    return lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz)


def tap_cell(i0, dims):
    """the macrocell (cx, cy, cz) whose value range covers the footprint (i0, i0 + 1) on every axis: min((i0 + 1) >> 4, cells - 1)"""
    n = np.asarray(dims, np.int64)
    return np.minimum((np.asarray(i0, np.int64) + 1) >> 4, (n + 15) // 16 - 1)


def macrocell_ranges(volume):
    """(mz, my, mx, 2): (min, max) of the 17 voxels from max(16 c - 1, 0) per axis (clipped to the volume) of every macrocell - the reference's ranges, which the
    upload computes -, in voxel_values' units"""
    v = voxel_values(volume)
    nz, ny, nx = v.shape
    mx, my, mz = (nx + 15) // 16, (ny + 15) // 16, (nz + 15) // 16
    out = np.empty((mz, my, mx, 2), F)
    for cz in range(mz):
        for cy in range(my):
            for cx in range(mx):
                bz, by, bx = max(16 * cz - 1, 0), max(16 * cy - 1, 0), max(16 * cx - 1, 0)
                b = v[bz:bz + 17, by:by + 17, bx:bx + 17]
                out[cz, cy, cx] = (np.nanmin(b), np.nanmax(b))
    return out


def slack(lo, hi):
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return fma(F(2.0 ** -21), ((hi - lo).astype(F) + fmax(np.abs(lo), np.abs(hi))).astype(F), FLT_MIN)


# ---- the three reductions --------------------------------------------------------------------------------------------------------------
def reduce(s, tm, count, mode):
    """s, tm (n, max_steps), count (n,) -> (v (n,), tm* (n,)); rays with count == 0 give the initial values"""
    s, tm = np.asarray(s, F), np.asarray(tm, F)
    n, width = s.shape
    valid = np.arange(width)[None, :] < np.asarray(count)[:, None]
    if mode == MEAN:
        acc = np.zeros((n, 4), F)
        for i in range(width):
            with np.errstate(invalid="ignore", over="ignore"):
                acc[:, i & 3] = np.where(valid[:, i], (acc[:, i & 3] + s[:, i]).astype(F), acc[:, i & 3])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v = (((acc[:, 0] + acc[:, 1]).astype(F) + (acc[:, 2] + acc[:, 3]).astype(F)).astype(F) / np.asarray(count).astype(F)).astype(F)
        return v, np.zeros(n, F)
    m = np.full(n, -np.inf if mode == MAXIMUM else np.inf, F)
    tb = np.zeros(n, F)
    for i in range(width):
        with np.errstate(invalid="ignore"):
            take = valid[:, i] & ((s[:, i] > m) if mode == MAXIMUM else (s[:, i] < m))
        m = np.where(take, s[:, i], m)
        tb = np.where(take, tm[:, i], tb)
    return m.astype(F), tb.astype(F)


def reduce_skipping(s, tm, count, lo, hi, mode):
    """the range-skipping reduction: lo, hi (n, max_steps) = the value range of each step's tap_cell.  Returns (v, tm*, fetched (n,)).  A skipped step's
    sample is never looked at; the bound is the extremum over the rounds before the step's own"""
    if mode == MEAN:
        v, tb = reduce(s, tm, count, mode)
        return v, tb, np.asarray(count).copy()
    s, tm = np.asarray(s, F), np.asarray(tm, F)
    n, width = s.shape
    valid = np.arange(width)[None, :] < np.asarray(count)[:, None]
    sl = slack(lo, hi)
    with np.errstate(invalid="ignore", over="ignore"):
        edge = (np.asarray(hi, F) + sl).astype(F) if mode == MAXIMUM else (np.asarray(lo, F) - sl).astype(F)
    m = np.full(n, -np.inf if mode == MAXIMUM else np.inf, F)
    tb = np.zeros(n, F)
    fetched = np.zeros(n, np.int64)
    for r0 in range(0, width, ROUND):
        bound = m.copy()
        for i in range(r0, min(r0 + ROUND, width)):
            with np.errstate(invalid="ignore"):
                cannot = (edge[:, i] <= bound) if mode == MAXIMUM else (edge[:, i] >= bound)
                fetch = valid[:, i] & ~cannot
                take = fetch & ((s[:, i] > m) if mode == MAXIMUM else (s[:, i] < m))
            fetched += fetch
            m = np.where(take, s[:, i], m)
            tb = np.where(take, tm[:, i], tb)
    return m.astype(F), tb.astype(F), fetched


# ---- the pixel -------------------------------------------------------------------------------------------------------------------------
def classify(v, colors, alphas, lower, upper):
    """v (n,) -> rgba (n, 4): colors (Nc, 3), alphas (Na,) - the tables as committed -, [lower, upper] the transfer function's range in the samples' units"""
    v = np.asarray(v, F).ravel()
    colors, alphas = np.asarray(colors, F).reshape(-1, 3), np.asarray(alphas, F).ravel()
    lower, upper = F(lower), F(upper)
    scale = F(0) if upper == lower else F(1) / F(upper - lower)
    with np.errstate(invalid="ignore", over="ignore"):
        c = clamp01(((fmin(fmax(v, lower), upper) - lower).astype(F) * scale).astype(F))
    out = np.empty((v.size, 4), F)
    for table, cols in ((colors, (0, 1, 2)), (alphas[:, None], (3,))):
        n1 = len(table) - 1
        x = (c * F(n1)).astype(F)
        i0 = x.astype(np.int64)
        f = (x - np.floor(x)).astype(F)
        i1 = np.minimum(i0 + 1, n1)
        for k, col in enumerate(cols):
            out[:, col] = lerp(table[i0, k], table[i1, k], f)
    out[:, :3] = clamp01(out[:, :3])
    return out


def normalized_range(value_range, dtype):
    """the transfer function's range in the samples' units: 8-bit types and 32-bit integers are normalised like their voxels"""
    lo, hi = (F(x) for x in value_range)
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return F(F(np.uint8(lo)) / F(255)), F(F(np.uint8(hi)) / F(255))
    if dt == np.int8:
        return max(F(F(np.int8(lo)) / F(127)), F(-1)), max(F(F(np.int8(hi)) / F(127)), F(-1))
    return lo, hi


# ---- rays and frames -------------------------------------------------------------------------------------------------------------------
def project_rays(volume, org, direction, rate, mode, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None, skipping=False,
                 camera_kind=0):
    """world rays org, direction (n, 3) - the direction used as given - -> dict(v, tm, steps, fetched, marched): what ovr_hip_project_floats returns
    (zeros for a ray that is not marched).  clip = (lo, hi): the OBJECT box; sampler(po) -> samples replaces the model's own tap (tests pass the oracle's);
    camera_kind = camera.ORTHOGRAPHIC: the rays are that camera's primary rays (camera.hits: a ray outside an ignored slab misses)"""
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
    tm, count = steps(t0, t1, F(1) / F(rate), hit)
    n, width = tm.shape
    with np.errstate(invalid="ignore", over="ignore"):
        pos = fma(np.nan_to_num(tm)[:, :, None], direction[:, None, :], org[:, None, :])
        po = clipping.to_object(pos.reshape(-1, 3), inv, wp)
    s = (sample(vol, po, vertex_centred) if sampler is None else np.asarray(sampler(po), F)).reshape(n, width)
    if skipping and mode != MEAN:
        i0, _ = tap_coordinates(po, dims, vertex_centred)
        c = tap_cell(i0, dims)
        rng = macrocell_ranges(vol)[c[:, 2], c[:, 1], c[:, 0]].reshape(n, width, 2)
        v, tb, fetched = reduce_skipping(s, tm, count, rng[..., 0], rng[..., 1], mode)
    else:
        v, tb = reduce(s, tm, count, mode)
        fetched = count.copy()
    marched = hit & (count > 0)
    z = F(0)
    return dict(v=np.where(marched, v, z).astype(F), tm=np.where(marched, tb, z).astype(F), steps=np.where(marched, count, 0), fetched=np.where(marched, fetched, 0),
                marched=marched, rays_hit=hit)


def frame(volume, basis, size, rate, mode, colors, alphas, tf_range, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, clip=None, sampler=None,
          skipping=False, spp=1, noise=None, frame_index=1, camera_kind=0):
    """one projection frame: rgba (H, W, 4), layer (H, W, 3) and counters.  basis = (pos, dir, hor, ver); tf_range in the samples' units (normalized_range);
    noise = the blue-noise tile ([y][x][t]) switches that jitter on - without it spp must be 1 (the RandomTEA jitter is not restated here);
    camera_kind = camera.ORTHOGRAPHIC: the basis is an orthographic camera's and the rays come from camera.pixel_rays (the default: today's rays, bit for bit)"""
    w, h = size
    if noise is None and spp != 1:
        raise ValueError("without the blue-noise jitter the model forms the rays of one sample per pixel")
    rgba, layer = np.zeros((h * w, 4), F), np.zeros((h * w, 3), F)
    counters = dict(rays=0, active_pixels=h * w, steps=0, fetched=0)
    org = np.broadcast_to(np.asarray(basis[0], F), (h * w, 3))
    for k in range(spp):
        xi = None if noise is None else blue_noise_variates(noise, w, h, frame_index, spp, k)
        d = pixel_rays(basis, w, h, xi).reshape(-1, 3)
        if camera_kind:
            from . import camera
            org, d = (a.reshape(-1, 3) for a in camera.pixel_rays(basis, w, h, xi, camera_kind))
        r = project_rays(volume, org, d, rate, mode, spacing, origin, vertex_centred, clip, sampler, skipping, camera_kind)
        m = r["marched"]
        c = classify(r["v"], colors, alphas, *tf_range)
        rgba = (rgba + np.where(m[:, None], c, F(0))).astype(F)
        layer = (layer + np.where(m[:, None], np.stack([r["v"], r["tm"], np.ones(h * w, F)], 1), F(0))).astype(F)
        counters["rays"] += h * w
        counters["steps"] += int(r["steps"].sum())
        counters["fetched"] += int(r["fetched"].sum())
    rspp = F(1) / F(spp)
    return (rgba * rspp).astype(F).reshape(h, w, 4), (layer * rspp).astype(F).reshape(h, w, 3), counters
