"""The convergence estimate of the HIP backend (include/ovr_hip.h, ovr_hip_set_convergence) as a numpy model.

While frames accumulate the renderer keeps, beside the running sum A of all frames, the sum H of the even-numbered
ones.  After an even frame n it compares the mean of all frames with the mean of that half, per pixel

    m_c = A_c / n        h_c = H_c / (n / 2)                      c = r, g, b, a
    d   = ((|m_r - h_r| + |m_g - h_g|) + |m_b - h_b|) + |m_a - h_a|
    s   = ((m_r + m_g) + m_b) + m_a
    e   = d / sqrt(s)  if s > 0  else 0

and per 8x8-pixel block E_b = T(e) / P, where T sums the block's 64 values with a balanced pairwise tree in the order
8 * (y & 7) + (x & 7) and P counts the pixels of the block that are inside the image and belong to the renderer (an
image shard draws some tiles only); the others contribute 0.  The frame error is the largest E_b.  Two halves of a
converged image agree, so the number falls towards 0 as frames accumulate; it has the shape of OSPRay's tile error
and is not claimed to equal its value.  Every step is IEEE float32 in exactly this order: the kernels reproduce
these functions bit for bit (tests/test_convergence_gpu.py).

Adaptive refinement retires a block after the first even frame at which E_b <= threshold: it is no longer marched
and is shown as A / n_b from then on (`retirement_frames`)."""
import numpy as np

BLOCK = 8


def owned_mask(width, height, rank=0, world=1, tile_w=64, tile_h=64):
    """(H, W) bool: the pixels an image shard draws, owner(tile) = (tile_x + tile_y) % world"""
    y, x = np.mgrid[0:height, 0:width]
    if world <= 1:
        return np.ones((height, width), bool)
    return ((x // tile_w + y // tile_h) % world) == rank


def pixel_errors(A, H, n):
    """e per pixel, (H, W) float32, from the (H, W, 4) float32 buffers after the even frame n"""
    if n < 2 or n % 2:
        raise ValueError("the estimate is defined after an even number of frames")
    A = np.asarray(A, np.float32)
    H = np.asarray(H, np.float32)
    m = A / np.float32(n)
    h = H / np.float32(n // 2)
    t = np.abs(m - h)
    d = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
    s = ((m[..., 0] + m[..., 1]) + m[..., 2]) + m[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d / np.sqrt(s)
    return np.where(s > 0, e, np.float32(0)).astype(np.float32)


def tree_sum(x):
    """balanced pairwise sum over the last axis (length 64), float32: six rounds of x[0::2] + x[1::2] - what a butterfly of
    shuffles over the lanes of a wave computes"""
    x = np.asarray(x, np.float32)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def block_errors(A, H, n, owned=None):
    """E_b as (ceil(H / 8), ceil(W / 8)) float32; owned: (H, W) bool, default every pixel"""
    e = pixel_errors(A, H, n)
    hh, ww = e.shape
    present = np.ones((hh, ww), bool) if owned is None else np.asarray(owned, bool)
    by, bx = (hh + BLOCK - 1) // BLOCK, (ww + BLOCK - 1) // BLOCK
    ep = np.zeros((by * BLOCK, bx * BLOCK), np.float32)
    pp = np.zeros((by * BLOCK, bx * BLOCK), bool)
    ep[:hh, :ww] = np.where(present, e, np.float32(0))
    pp[:hh, :ww] = present
    # lane = 8 * (y & 7) + (x & 7)
    lanes = ep.reshape(by, BLOCK, bx, BLOCK).transpose(0, 2, 1, 3).reshape(by, bx, BLOCK * BLOCK)
    count = pp.reshape(by, BLOCK, bx, BLOCK).transpose(0, 2, 1, 3).reshape(by, bx, BLOCK * BLOCK).sum(-1)
    t = tree_sum(lanes)
    with np.errstate(divide="ignore", invalid="ignore"):
        E = t / count.astype(np.float32)
    return np.where(count > 0, E, np.float32(0)).astype(np.float32)


def frame_error(A, H, n, owned=None):
    return np.float32(block_errors(A, H, n, owned).max())


def accumulate(frames):
    """[(n, A_n, H_n)] for n = 1 ... len(frames): the float32 running sums, added in frame order as the renderer does (H_1 = 0)"""
    A = None
    H = None
    out = []
    for k, f in enumerate(frames, 1):
        f = np.asarray(f, np.float32)
        A = f.copy() if A is None else A + f
        if k % 2 == 0:
            H = f.copy() if H is None else H + f
        out.append((k, A.copy(), np.zeros_like(A) if H is None else H.copy()))
    return out


def retirement_frames(frames, threshold, owned=None, eligible=None):
    """Simulates adaptive refinement on the per-frame images `frames[k - 1]` (frame k as rendered on its own): returns
    (n_b, E_b, image) - n_b (blocks,) int32: the even frame after which block b retired, 0 = still active after the last
    frame; E_b its last estimate; image = A_{n_b} / n_b for retired blocks, A_N / N for active ones.  eligible: (by, bx)
    bool, the blocks that are marched at all (a block no ray meets is never estimated)."""
    threshold = np.float32(threshold)
    sums = accumulate(frames)
    hh, ww = sums[0][1].shape[:2]
    by, bx = (hh + BLOCK - 1) // BLOCK, (ww + BLOCK - 1) // BLOCK
    n_b = np.zeros((by, bx), np.int32)
    E_b = np.zeros((by, bx), np.float32)
    elig = np.ones((by, bx), bool) if eligible is None else np.asarray(eligible, bool)
    N = len(frames)
    image = sums[-1][1] / np.float32(N) if N > 1 else sums[-1][1].copy()
    for n, A, H in sums:
        if n % 2:
            continue
        E = block_errors(A, H, n, owned)
        active = (n_b == 0) & elig
        E_b = np.where(active, E, E_b)
        now = active & (E <= threshold)
        n_b = np.where(now, n, n_b)
        mean = A / np.float32(n)
        for j, i in zip(*np.nonzero(now)):
            image[j * BLOCK:(j + 1) * BLOCK, i * BLOCK:(i + 1) * BLOCK] = mean[j * BLOCK:(j + 1) * BLOCK, i * BLOCK:(i + 1) * BLOCK]
    return n_b, E_b, image
