"""The shadow cache of the HIP backend (include/ovr_hip.h, ovr_hip_set_shadow_cache) as a numpy model: the normative text.

Full shading marches one shadow ray per shaded sample towards ONE directional light.  While the volume, the transfer function
and the light stand still the shadow term is a view-independent scalar field: it is computed once on a lattice and read back
with one trilinear tap.

Lattice: in the volume's object space, where the volume is the unit cube.  Per axis a with dim_a voxels and cell >= 1

    N_a = ceil(dim_a / cell) + 1                                 (`lattice_dims`)
    u_i = float32(i) / float32(N_a - 1)     i = 0 ... N_a - 1    (`node_coordinates`: an IEEE divide, the last node is exactly 1)
    w_i = fma(u_i, sc_a, origin_a)          sc_a = spacing_a * ext_a in float32, ext_a = dim_a (cell-centred) or dim_a - 1
                                                                 (`node_positions`: the world position the node's march starts from)

stored as N_x * N_y * N_z float32, x fastest - here arrays of shape (N_z, N_y, N_x).

Node value: S[node] is what the frame's own shadow march returns from the node's world position - the committed light direction,
sampling rate (stride 10 / rate^2), transfer function, grid convention and clip box, early termination at 0.9999 included.  The
model adds no arithmetic of its own there: the CPU oracle's march is the reference (tests/test_shadow_cache_gpu.py).

Lookup (`lookup`): for a shaded sample at the object position po (what the march's to_object makes of its world position)

    g_a = clamp01(po_a) * float32(N_a - 1)
    i_a = min(int(floor(g_a)), N_a - 2)
    f_a = g_a - float32(i_a)
    shadow = lerp along x, then y, then z of the cell's eight nodes,     lerp(a, b, f) = fma(f, b - a, a)

The result is not clamped.  clamp01 is clipping.clamp01 (NaN -> 0).  At a node whose coordinate comes back as g = i exactly (every
node when N - 1 is a power of two; the first and the last node of any axis) f is 0 and fma(0, b - a, a) = a: the node's bits.  On
an upper face i = N - 2 and f = 1: fma(1, b - a, a), which is b where b - a is exact and within an ulp of it otherwise.  A
constant lattice stays constant bit for bit (b - a = 0).

Quality: the lattice resolves shadows no finer than its cell; features thinner than a cell (thin shells) are smeared and the cached
term can be WORSE than no shadow term at all - DESIGN.md section 14 has the table."""
import numpy as np

from .clipping import clamp01
from .lighting import fma

F = np.float32
DEFAULT_CELL = 4


def lattice_dims(dims, cell):
    """(N_x, N_y, N_z) of a volume of dims = (nx, ny, nz) voxels"""
    cell = int(cell)
    if cell < 1:
        raise ValueError("the cell size is at least 1 voxel")
    return tuple((int(d) + cell - 1) // cell + 1 for d in dims)


def node_coordinates(n):
    """the object coordinate u_i of the n nodes of one axis"""
    return (np.arange(n, dtype=F) / F(n - 1)).astype(F)


def node_positions(dims, cell=DEFAULT_CELL, spacing=(1, 1, 1), origin=(0, 0, 0), vertex_centred=False, lattice=None):
    """world positions of the nodes, shape (N_z, N_y, N_x, 3); lattice = (N_x, N_y, N_z) overrides lattice_dims (a supplied lattice)"""
    n = lattice_dims(dims, cell) if lattice is None else tuple(int(x) for x in lattice)
    d = np.asarray(dims, np.int64)
    ext = (d - 1 if vertex_centred else d).astype(F)
    sc = (np.asarray(spacing, F) * ext).astype(F)
    org = np.asarray(origin, F)
    w = [fma(node_coordinates(n[k]), sc[k], org[k]) for k in range(3)]
    out = np.empty((n[2], n[1], n[0], 3), F)
    out[..., 0] = w[0][None, None, :]
    out[..., 1] = w[1][None, :, None]
    out[..., 2] = w[2][:, None, None]
    return out


def lerp(a, b, f):
    return fma(f, (np.asarray(b, F) - np.asarray(a, F)).astype(F), a)


def lookup(lattice, po):
    """lattice (N_z, N_y, N_x) float32, po (n, 3) object positions -> (n,) float32"""
    s = np.asarray(lattice, F)
    po = np.asarray(po, F).reshape(-1, 3)
    nz, ny, nx = s.shape
    idx, frac = [], []
    for k, n in enumerate((nx, ny, nz)):
        g = (clamp01(po[:, k]) * F(n - 1)).astype(F)
        i = np.minimum(np.floor(g).astype(np.int64), n - 2)
        idx.append(i)
        frac.append((g - i.astype(F)).astype(F))
    (ix, iy, iz), (fx, fy, fz) = idx, frac
    c00 = lerp(s[iz, iy, ix], s[iz, iy, ix + 1], fx)
    c10 = lerp(s[iz, iy + 1, ix], s[iz, iy + 1, ix + 1], fx)
    c01 = lerp(s[iz + 1, iy, ix], s[iz + 1, iy, ix + 1], fx)
    c11 = lerp(s[iz + 1, iy + 1, ix], s[iz + 1, iy + 1, ix + 1], fx)
    return lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz)


def partner_rate(rate):
    """the sampling rate r' at which the unshaded PRIMARY march steps like the shadow march of a renderer at `rate`: step' = 1 / r' must equal
    the shadow stride (1 / rate * 10) * (1 / rate) in float32 - r' = float32(rate * rate / 10) does for the rates `partner_rate_exact` accepts"""
    return F(F(rate) * F(rate) / F(10))


def shadow_stride(rate):
    step = F(1) / F(rate)
    return F(F(step * F(10)) * step)


def partner_rate_exact(rate):
    return bool(F(1) / partner_rate(rate) == shadow_stride(rate))
