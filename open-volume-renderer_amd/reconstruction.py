"""Pull-push reconstruction of sparse-sampled frames in numpy: the normative text of ovr_hip_set_reconstruction (include/ovr_hip.h, DESIGN.md
section 10).  The HIP kernels (ovr_hip_kernels.hip, recon_*) are held to this file bit for bit, so it is written to be read, operation by operation.

A frame has up to seven channels per pixel - r, g, b, a of the RGBA layer (premultiplied, so interpolating them is sound) and the three of the gradient
layer - and a weight plane: weight > 0 means "this pixel was sampled".  All arithmetic is IEEE float32, every *, +, / rounded on its own, in the order
written; where a value does not take part, +0 is SELECTED in its place (np.where), it is never multiplied by 0.

    level 0   v0 = the image; w0 = 1 where the pixel was sampled and all its channels are finite, else 0
    pull      level l + 1 has ceil(W / 2) x ceil(H / 2) texels, until 1 x 1.  Children c0 .. c3 = (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1);
              s = (w0 + w1) + (w2 + w3);  t = (u0 + u1) + (u2 + u3) per channel with u_i = w_i == 1 ? v_i : +0;  v' = s > 0 ? t / s : +0;  w' = s > 0
    push      from the 1 x 1 level down: a texel with w == 1 keeps its value; the others take U, the bilinear interpolation of the completed coarser
              level P:  px = x >> 1, nx = clamp(px + (x odd ? 1 : -1)), the same in y,
              a = 0.75 P(px, py) + 0.25 P(nx, py);  b = 0.75 P(px, ny) + 0.25 P(nx, ny);  U = 0.75 a + 0.25 b
              On level 0 the test is "sampled", not w0 == 1: a sampled pixel with a non-finite channel keeps its value and spreads nowhere.

The weight of a texel saturates (0 or 1) on purpose: averaging the weights instead lets a 7 % sampling density pull the whole picture towards its mean.
"""
import numpy as np

F = np.float32


def levels(width, height):
    """[(W_l, H_l)] from the image down to 1 x 1"""
    out = [(int(width), int(height))]
    while out[-1][0] > 1 or out[-1][1] > 1:
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def level0(accum, grad_sum, count):
    """level 0 of an accumulating renderer: N > 0 ? (A / N, G / N) : 0 per channel (IEEE division; a select, never 0 * x)"""
    n = np.asarray(count, F)
    has = n > 0
    safe = np.where(has, n, F(1))[..., None]
    with np.errstate(all="ignore"):
        rgba = np.where(has[..., None], np.asarray(accum, F) / safe, F(0)).astype(F)
        grad = None if grad_sum is None else np.where(has[..., None], np.asarray(grad_sum, F) / safe, F(0)).astype(F)
    return rgba, grad


def pull(v, w):
    """one level up: v (H, W, C) float32, w (H, W) float32 of 0 / 1 -> (v', w')"""
    h, wd, c = v.shape
    h2, w2 = (h + 1) // 2, (wd + 1) // 2
    u = np.zeros((2 * h2, 2 * w2, c), F)  # children outside the level: weight 0, value +0
    wp = np.zeros((2 * h2, 2 * w2), F)
    u[:h, :wd] = np.where((w == 1)[..., None], v, F(0))
    wp[:h, :wd] = w
    with np.errstate(all="ignore"):
        s = (wp[0::2, 0::2] + wp[0::2, 1::2]) + (wp[1::2, 0::2] + wp[1::2, 1::2])
        t = (u[0::2, 0::2] + u[0::2, 1::2]) + (u[1::2, 0::2] + u[1::2, 1::2])
        has = s > 0
        out = np.where(has[..., None], t / np.where(has, s, F(1))[..., None], F(0)).astype(F)
    return out, has.astype(F)


def upsample(p, width, height):
    """U for every texel of a width x height level from the completed coarser level p (H', W', C)"""
    hc, wc, _ = p.shape
    x, y = np.arange(width), np.arange(height)
    px, py = x >> 1, y >> 1
    nx = np.clip(px + np.where(x & 1, 1, -1), 0, wc - 1)
    ny = np.clip(py + np.where(y & 1, 1, -1), 0, hc - 1)
    with np.errstate(all="ignore"):
        a = F(0.75) * p[py][:, px] + F(0.25) * p[py][:, nx]
        b = F(0.75) * p[ny][:, px] + F(0.25) * p[ny][:, nx]
        return (F(0.75) * a + F(0.25) * b).astype(F)


def reconstruct(rgba, grad, weight):
    """rgba (H, W, 4), grad (H, W, 3) or None, weight (H, W): > 0 = sampled  ->  (rgba, grad) filled; grad is None when none was given"""
    rgba = np.ascontiguousarray(rgba, F)
    h, w = rgba.shape[:2]
    v0 = rgba if grad is None else np.concatenate([rgba, np.ascontiguousarray(grad, F).reshape(h, w, 3)], axis=2)
    sampled = np.asarray(weight).reshape(h, w) > 0
    w0 = (sampled & np.isfinite(v0).all(axis=2)).astype(F)
    vs, ws = [v0], [w0]
    while vs[-1].shape[0] > 1 or vs[-1].shape[1] > 1:
        v, wt = pull(vs[-1], ws[-1])
        vs.append(v)
        ws.append(wt)
    # the 1 x 1 level is complete as it is (0 when the frame had no finite sample); on level 0 a hole of a 1 x 1 image is 0 as well
    done = np.where(sampled[..., None], v0, F(0)).astype(F) if len(vs) == 1 else vs[-1]
    for l in range(len(vs) - 2, -1, -1):
        keep = sampled if l == 0 else ws[l] == 1
        u = upsample(done, vs[l].shape[1], vs[l].shape[0])
        done = np.where(keep[..., None], vs[l], u).astype(F)
    if grad is None:
        return done, None
    return np.ascontiguousarray(done[..., :4]), np.ascontiguousarray(done[..., 4:])
