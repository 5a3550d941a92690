"""The eight newer frame kinds under the host machinery every frame runs through (host/frame.cpp, ovr_hip_device.h): a fixed matrix, the
kinds of tests/frame_machinery_cases.py by

  A  the dense frame against the kind's model, through the feature test's own _check_frame at its own bars - what anchors every equality below
  B  sparse sampling: the CPU oracle's sample list; listed pixels are the dense frame's, every other pixel is 0, in both framebuffer sets
  C  sparse sampling + FILL: the whole frame is reconstruction.reconstruct(OFF frame, OFF layer, list), the counters are the OFF run's
  D  sparse sampling + FILL + accumulation, frames 1 ... 4: N, G and the frame as tests/test_reconstruction_gpu.py::test_accumulated_sparse_frames holds the march
  E  three image shards of 16 x 8 tiles assemble to the single renderer's frame, and so does a device group [0, 0, 0]
  F  ESTIMATE changes no frame, layer or counter, and its block errors are convergence.block_errors of the renderer's own A and H
  G  ADAPTIVE: a non-accumulating twin's frames S_k and convergence.retirement_frames predict the retirement frames, the errors, A_{n_b} / n_b in both
     framebuffer sets, the layer a retiring block keeps (S_{n_b}'s) and the rays counted - under a threshold taken from the MODEL's frames, not the device's
  H  ovr_hip_update_volume of an unaligned box against a fresh renderer given the patched volume, and against the model of the patched volume

one renderer, or a pair, per cell.  Everything is compared bit for bit ("bits": float32 bit patterns) but what goes through an imported _check_frame; there is
no tolerance of this file's own.  The layer's rule, which the depth layer (d, S, reached) shares with the gradient layer: it is the last frame's value, a retiring
block keeps the one of its retirement frame, and under accumulated FILL it is G / N.  tests/test_frame_machinery_model.py shows without a GPU that the
conditions asserted here (lists with holes, lit frames, blocks that retire late and blocks that stay, a box that changes the frame) hold for the models.

Durations on the MI355X (pytest --durations=0, call phase): the 64 cells take 4.6 s together.  The first cell of a session 1.6 s (it loads the library and
creates the first context); G 0.03 - 0.24 s per kind (gradient 0.24, limited 0.18, depth-limited 0.17, preintegrated and slab 0.10: eight model frames for the
threshold, sixteen rendered frames); H at most 0.06 s, A at most 0.05 s, every cell of B, C, D, E and F at most 0.02 s; the teardown of an E cell, which closes a
group of three, 0.02 s.

What a wrong reference does to the columns (tests the tests; run once by hand, references mutated, device code untouched): the oracle's list taken one frame
index late fails all 8 cells of B; A / n in place of A / N in reconstruction.level0 all 8 of D; the last frame's layer in place of the one kept at retirement 7
of 8 of G (the pre-integrated frame's layer is zero: it cannot tell); a twin patched one voxel off in x all 8 of H."""
import numpy as np
import pytest

import frame_machinery_cases as FM
import test_convergence_gpu as TC
import test_reconstruction_gpu as TR
from helpers import hip_frame

pytestmark = pytest.mark.gpu
f32 = np.float32
KINDS = pytest.mark.parametrize("kind", FM.KINDS, ids=FM.IDS)
PICTURE = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples", "pipeline", "layout", "skipping_kernels")
_dense = {}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _counters(st, names):
    return {k: int(getattr(st, k)) for k in names}


@pytest.fixture
def made(ovr):
    rs = []

    def make(**kw):
        r = ovr.create_renderer("hip", **kw)
        rs.append(r)
        return r

    yield make
    for r in rs:
        r.close()


def _render(ovr, ren):
    ren.render()
    rgba, layer = hip_frame(ovr, ren)
    return rgba, layer, ren.stats()


def _dense_frame(ovr, oracle, made, kind, size):
    """the kind's dense frame (rgba, layer, stats) of a renderer of its own, once per session; at the small size it is held to the kind's model here, so that
    whichever test asks for it first anchors it"""
    key = (kind.key, size)
    if key not in _dense:
        case = kind.case(ovr, size)
        ren = kind.begin(ovr, made(), case)
        got = _render(ovr, ren)
        if size == FM.SMALL:
            kind.check(ovr, oracle, ren, case, got, FM.model_frame(ovr, kind, size, ren=ren), (kind.name, "dense"))
        lit = int((got[0][..., 3] > 0).sum())
        assert FM.LIT_PIXELS < lit < size[0] * size[1] and got[1].any() == (kind.layer != "zero"), (kind.name, lit)
        if kind.plane:      # the depth image is the one of the whole frame
            g, image = ren.get_max_depth(values=True)
            assert (g.active, g.width, g.height) == (1,) + size and _same(image, kind.depth(size))
        _dense[key] = got
    return _dense[key]


def _sparse(ovr, made, kind, case, mode, accumulate=False):
    ren = kind.begin(ovr, made(), case, accumulate=accumulate, noise=True)
    ren.set_focus(*FM.FOCUS)
    ren.set_sparse_sampling(True)
    ren.set_reconstruction(mode)
    ren.commit()
    return ren


# ---- A. the dense frame is the model's -----------------------------------------------------------------------------------------------------------------------

@KINDS
def test_dense_frame_against_the_model(ovr, oracle, made, kind):
    got = _dense_frame(ovr, oracle, made, kind, FM.SMALL)
    if kind.layer == "depth":
        reached = got[1][..., 2] == 1
        assert reached.sum() > 50 and ((got[0][..., 3] > 0) & ~reached).sum() > 50
    if kind.skipping and kind.name == "slab":
        assert got[2].skipping_kernels == 1      # the walk kernel's skipping twin drew it


# ---- B. sparse sampling ----------------------------------------------------------------------------------------------------------------------------------------

@KINDS
def test_sparse_sampling(ovr, oracle, made, kind):
    dense = _dense_frame(ovr, oracle, made, kind, FM.SMALL)
    w, h = FM.SMALL
    ren = _sparse(ovr, made, kind, kind.case(ovr, FM.SMALL), 0)
    if kind.plane:
        g = ren.get_max_depth()
        assert (g.active, g.width, g.height) == (1, w, h)      # the full-size image under a list of pixels
    for k in (1, 2):
        rgba, layer, st = _render(ovr, ren)
        assert st.frame_index == k
        m = FM.indicator(oracle, k, FM.SMALL)
        s = m > 0
        xy = ren.sparse_mask(k).reshape(-1, 2)
        mine = np.zeros((h, w), f32)
        mine[xy[:, 1], xy[:, 0]] = 1
        assert len(xy) == int(m.sum()) and np.array_equal(mine, m), f"frame {k}: the device's list is not the oracle's"
        assert _same(rgba[s], dense[0][s]) and _same(layer[s], dense[1][s]), f"frame {k}: a listed pixel is not the dense frame's"
        assert not rgba[~s].any() and not layer[~s].any(), f"frame {k}: a pixel outside the list was written"
        assert st.active_pixels == int(m.sum()) and 50 <= int(m.sum()) <= w * h - 50
        assert rgba[s].any() and (layer[s].any() or kind.layer == "zero")
        ren.swap()


# ---- C. sparse sampling + FILL ---------------------------------------------------------------------------------------------------------------------------------

@KINDS
def test_sparse_frames_are_filled_as_the_model_says(ovr, oracle, made, kind):
    M = ovr.reconstruction
    w, h = FM.SMALL
    case = kind.case(ovr, FM.SMALL)
    fill, off = _sparse(ovr, made, kind, case, 1), _sparse(ovr, made, kind, case, 0)
    for k in (1, 2):
        f, o = _render(ovr, fill), _render(ovr, off)
        assert f[2].frame_index == o[2].frame_index == k
        m = FM.indicator(oracle, k, FM.SMALL)
        want_rgba, want_layer = M.reconstruct(o[0], o[1], m)
        assert _same(f[0], want_rgba) and _same(f[1], want_layer), f"frame {k}: the filled frame is not the model's"
        assert _same(fill.reconstruction_weights(), m)
        r = fill.reconstruction()
        assert r.mode == 1 and r.valid == 1 and r.sampled_pixels == int(m.sum()) and r.filled_pixels == w * h - int(m.sum()) and off.reconstruction().valid == 0
        assert _counters(f[2], TR.COUNTERS) == _counters(o[2], TR.COUNTERS)
        assert (f[0][..., 3] > 0).sum() > (o[0][..., 3] > 0).sum()      # holes were filled
        if kind.layer != "zero":
            assert f[1][m == 0].any()      # ... of the layer too
        fill.swap()
        off.swap()


# ---- D. sparse sampling + FILL + accumulation --------------------------------------------------------------------------------------------------------------------

@KINDS
def test_accumulated_sparse_frames(ovr, oracle, made, kind):
    """tests/test_reconstruction_gpu.py::test_accumulated_sparse_frames on the kind: N is the per-pixel count of the oracle's lists, G the sum, in frame order, of
    the layer pixels the OFF run's frames show at the listed pixels, the frame model(A / N, G / N, N) with A read back from the renderer"""
    M = ovr.reconstruction
    w, h = FM.SMALL
    case = kind.case(ovr, FM.SMALL)
    fill, off = _sparse(ovr, made, kind, case, 1, accumulate=True), _sparse(ovr, made, kind, case, 0, accumulate=True)
    N, G = np.zeros((h, w), f32), np.zeros((h, w, 3), f32)
    for k in range(1, FM.SPARSE_FRAMES + 1):
        f, o = _render(ovr, fill), _render(ovr, off)
        assert f[2].frame_index == o[2].frame_index == k
        m = FM.indicator(oracle, k, FM.SMALL)
        s = m > 0
        N += m
        G[s] = (G[s] + o[1][s]).astype(f32)
        assert _same(fill.reconstruction_weights(), N), f"frame {k}: N is not the count of the oracle's lists"
        assert _same(fill.reconstruction_gradient(), G), f"frame {k}: G is not the sum of the OFF run's layer pixels"
        A = fill.accumulation(0)
        assert _same(A, off.accumulation(0))
        want_rgba, want_layer = M.reconstruct(*M.level0(A, G, N), N)
        assert _same(f[0], want_rgba) and _same(f[1], want_layer), f"frame {k}: the filled frame is not the model's"
        r = fill.reconstruction()
        assert r.valid == 1 and r.sampled_pixels == int((N > 0).sum())
        assert _same(f[0][N > 0], (A[N > 0] / N[N > 0][:, None]).astype(f32))      # a listed pixel shows A / N, not the OFF run's A / k
        fill.swap()
        off.swap()
    assert N.max() >= 2 and (N == 0).any() and A.any() and (G.any() or kind.layer == "zero")


# ---- E. image shards and a device group --------------------------------------------------------------------------------------------------------------------------

def _totals(st):
    return np.array((st.rays, st.samples + st.skipped_samples, st.shaded_samples, st.active_pixels), np.int64)


@KINDS
def test_image_shards_and_a_device_group_of_three(ovr, oracle, made, kind):
    size, (tw, th) = FM.LARGE, FM.TILE
    whole = _dense_frame(ovr, oracle, made, kind, size)
    case = kind.case(ovr, size)
    ys, xs = np.mgrid[0:size[1], 0:size[0]]
    owner = ((xs // tw) + (ys // th)) % FM.WORLD
    assert all((owner == rank).sum() > 500 for rank in range(FM.WORLD))
    rgba, layer = np.full_like(whole[0], np.nan), np.full_like(whole[1], np.nan)
    totals = np.zeros(4, np.int64)
    for rank in range(FM.WORLD):
        ren = made()
        ren.set_image_shard(rank, FM.WORLD, tw, th)
        part = _render(ovr, kind.begin(ovr, ren, case))
        rgba[owner == rank], layer[owner == rank] = part[0][owner == rank], part[1][owner == rank]
        totals += _totals(part[2])
        if kind.plane:      # every rank holds the image of the whole frame
            g = ren.get_max_depth()
            assert (g.active, g.width, g.height) == (1,) + size
    assert _same(rgba, whole[0]) and _same(layer, whole[1]), "the ranks' pixels do not assemble to the single renderer's frame"
    assert np.array_equal(totals, _totals(whole[2])), (totals, _totals(whole[2]))
    group = made(devices=[0] * FM.WORLD)
    kind.begin(ovr, group, case)
    group.set_image_shard(0, 1, tw, th)
    group.commit()
    g = _render(ovr, group)
    assert _same(g[0], whole[0]) and _same(g[1], whole[1]), "the group's frame is not the single renderer's"
    assert np.array_equal(_totals(g[2]), _totals(whole[2])), (_totals(g[2]), _totals(whole[2]))


# ---- F. ESTIMATE -------------------------------------------------------------------------------------------------------------------------------------------------

@KINDS
def test_estimate_changes_nothing_and_is_the_model(ovr, made, kind):
    M = ovr.convergence
    w, h = FM.SMALL
    case = kind.case(ovr, FM.SMALL)
    rens = []
    for mode in (0, 1):
        ren = kind.begin(ovr, made(), case, accumulate=True, jitter=True)
        ren.set_convergence(mode)
        ren.commit()
        rens.append(ren)
    plain, est = rens
    first = None
    for n in range(1, FM.ESTIMATE_FRAMES + 1):
        a, b = _render(ovr, plain), _render(ovr, est)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), f"frame {n}: the estimate changed the frame"
        assert _counters(a[2], TC.COUNTERS) == _counters(b[2], TC.COUNTERS) and a[2].frame_index == n
        first = a if first is None else first
        if n % 2 == 0:
            err, frames = est.convergence_blocks()
            want = M.block_errors(est.accumulation(0), est.accumulation(1), n)
            assert err.shape == want.shape == ((h + 7) // 8, (w + 7) // 8) and _same(err, want), f"frame {n}: {int((err != want).sum())} block errors differ from the model"
            assert set(np.unique(frames)) <= {0, n} and np.all(frames[want > 0] == n) and (want > 0).sum() >= 4
            c = est.convergence()
            assert c.valid == 1 and c.frames == n and f32(c.error) == err.max() > 0
        plain.swap()
        est.swap()
    assert not _same(a[0], first[0]) and (kind.layer == "zero" or not _same(a[1], first[1]))      # the jitter moved the frames: H is not A / 2


# ---- G. ADAPTIVE -------------------------------------------------------------------------------------------------------------------------------------------------

def _blocks(n_b, size):
    """the per-block plane as (H, W)"""
    return np.repeat(np.repeat(n_b, 8, axis=0), 8, axis=1)[:size[1], :size[0]]


def _kept_layer(layers, n_b, last, size):
    """the layer after frame `last`: frame last's, and for a block retired after frame n_b the one of frame n_b"""
    px = _blocks(n_b, size)
    out = layers[last - 1].copy()
    for n in np.unique(n_b[n_b > 0]):
        out[px == n] = layers[n - 1][px == n]
    return out


@KINDS
def test_adaptive_refinement_is_predicted_by_the_single_frames(ovr, made, kind):
    M = ovr.convergence
    size, N = FM.LARGE, FM.ADAPTIVE_FRAMES
    w, h = size
    case = kind.case(ovr, size)
    # the threshold: from the MODEL's frames 1 ... 4 (tests/test_frame_machinery_model.py holds the condition below for the model's own frames under it)
    t = FM.threshold(ovr, kind, [FM.model_frame(ovr, kind, size, k)[0] for k in range(1, FM.THRESHOLD_FRAME + 1)])
    # S_k: frame k as a non-accumulating renderer draws it - the same frame_index, hence the same jitter
    single = kind.begin(ovr, made(), case, jitter=True)
    S = []
    for k in range(1, N + 1):
        rgba, layer, st = _render(ovr, single)
        assert st.frame_index == k and st.rays == w * h
        S.append((rgba, layer))
        single.swap()
    fr, layers = [s[0] for s in S], [s[1] for s in S]
    assert not _same(fr[0], fr[1])
    hit = FM.block_hit(fr)
    ren = kind.begin(ovr, made(), case, accumulate=True, jitter=True)
    ren.set_convergence(2, t)
    ren.commit()
    marched_before = None
    for n in range(1, N + 1):
        rgba, layer, st = _render(ovr, ren)
        assert st.frame_index == n
        if n == 1:
            assert st.rays == w * h and _same(rgba, fr[0]) and _same(layer, layers[0])
        elif n % 2:
            assert st.rays == 64 * int(marched_before.sum()), n
        else:
            err, frames = ren.convergence_blocks()
            want_nb, want_E, want_img = M.retirement_frames(fr[:n], t)
            got_nb = np.where(frames < 0, -frames, 0)
            assert np.array_equal(got_nb[hit], want_nb[hit]) and np.isin(got_nb[~hit], (0, 2)).all(), (n, got_nb.tolist(), want_nb.tolist())
            assert _same(err[hit], want_E[hit]) and not err[~hit].any(), n
            assert set(np.unique(frames[frames >= 0])) <= {0, n}
            marched = (frames == 0) | (np.abs(frames) == n)      # never estimated (no ray lights them: they keep counting), or marched by this frame
            assert st.rays == 64 * int(marched.sum()), n
            marched_before = (frames == 0) | (frames == n)
            assert _same(rgba, want_img) and _same(layer, _kept_layer(layers, want_nb, n, size)), n
        if n < N:
            ren.swap()
    # after frame N: the condition, the counts, and both framebuffer sets
    retired, late, active = FM.adaptive_condition(got_nb, hit, N)
    print(kind.name, "threshold", t, "lit blocks", int(hit.sum()), "retired", retired, "later than frame 2", late, "active", active)
    c = ren.convergence()
    assert c.valid == 1 and c.frames == N and c.retired_blocks == int((frames < 0).sum()) and c.active_blocks == int((frames == N).sum()) and c.blocks == c.retired_blocks + c.active_blocks
    assert np.all(err[frames < 0] <= f32(t)) and np.all(err[frames == N] > f32(t))
    A = ren.accumulation(0)
    n_px = _blocks(np.where(got_nb > 0, got_nb, N), size).astype(f32)
    assert _same(rgba, (A / n_px[..., None]).astype(f32))      # (A stops growing where a block retired)
    assert not _same(_kept_layer(layers, want_nb, N, size), layers[N - 1]) or kind.layer == "zero"      # a kept layer differs from the last frame's: the rule is seen
    ren.swap()      # the other set holds frame N - 1: the same rule one frame earlier
    other_nb, _, other_img = M.retirement_frames(fr[:N - 1], t)
    rgba, layer = hip_frame(ovr, ren)
    assert _same(rgba, other_img) and _same(layer, _kept_layer(layers, other_nb, N - 1, size))


# ---- H. ovr_hip_update_volume --------------------------------------------------------------------------------------------------------------------------------------

@KINDS
def test_update_volume_against_a_fresh_twin_and_the_model(ovr, oracle, made, kind):
    row = kind.update
    vol = row.volume()
    patch, patched = FM.patch_volume(vol, row.patch)
    case, twin_case = row.case(ovr, FM.SMALL), row.case(ovr, FM.SMALL, patched)
    ren = row.begin(ovr, made(), case)
    before = _render(ovr, ren)
    pre = None
    if row.name == "preintegrated":
        g = ren.get_preintegration()
        pre = ((g.mode, g.active, g.nodes, g.subdivision), np.array(ren.preintegration_tables(), copy=True))
    ren.update_volume(patch, FM.BOX_LOWER)
    after = _render(ovr, ren)
    twin = row.begin(ovr, made(), twin_case)
    fresh = _render(ovr, twin)
    assert _same(after[0], fresh[0]) and _same(after[1], fresh[1]), (row.key, "the updated renderer's frame is not the fresh one's")
    assert _counters(after[2], PICTURE) == _counters(fresh[2], PICTURE)
    row.check(ovr, oracle, ren, twin_case, after, FM.model_frame(ovr, row, FM.SMALL, vol=patched, ren=ren), (row.name, "patched"))
    changed = int(((_bits(after[0]) != _bits(before[0])).any(-1) | (_bits(after[1]) != _bits(before[1])).any(-1)).sum())
    assert changed > FM.UPDATE_PIXELS, (row.key, changed)
    if row.skipping:
        assert ren.slices().range_skipping == twin.slices().range_skipping == int(row.name == "slab") and after[2].skipping_kernels == int(row.name == "slab")
    if pre is not None:      # the node table depends on the transfer function alone
        g = ren.get_preintegration()
        assert (g.mode, g.active, g.nodes, g.subdivision) == pre[0] and _same(ren.preintegration_tables(), pre[1])
