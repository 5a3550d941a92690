"""The signed voxel types (int8, int16) in the numpy models, on the CPU: projection.sample, classify under normalized_range and the step counts against the
unmodified oracle; isosurface.trace_rays against a float64 walk of the signed field; the side a skipped cell is given, by brute force over the oracle's ranges;
product_sampler(int8) against the per-voxel-normalised tap.  Then the conditions that keep tests/test_signed_types_gpu.py discriminating: a tap without the
int8 clamp of -128 to -127, and a tap that reads the voxels as unsigned, change what those tests compare.  No GPU."""
import numpy as np
import pytest

import isosurface_cases as IC
import projection_cases as PC
import signed_cases as SC
from test_projection_model import _dense_positions, _scene

F = np.float32
U = 2.0 ** -24
IDS = lambda d: np.dtype(d).name


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


# ---- 1. the models against the unmodified oracle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("convention", (0, 1), ids=("cell", "vertex"))
@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_samples_are_the_oracles_bit_for_bit(ovr, oracle, dtype, convention):
    """blocks of the type's minimum next to minimum + 1: for int8 both are -1.0 behind the clamp, for int16 they differ by one"""
    P = ovr.projection
    vol = SC.minimum_blocks(dtype)
    lowest = SC.MINIMUM[np.dtype(dtype)]
    assert (vol == lowest).sum() >= 400 and (vol == lowest + 1).sum() >= 400
    nz, ny, nx = vol.shape
    sc = _scene(oracle, ovr, vol, convention=convention)
    rng = np.random.default_rng(23)
    po = (rng.random((1500, 3)) * 1.1 - 0.05).astype(F)
    po[:700] = ((np.array([4.0, 2.0, 1.0]) + rng.random((700, 3)) * np.array([20.0, 14.0, 9.0])) / np.array([nx, ny, nz])).astype(F)      # in and around the blocks
    po[700:900, 0] = ((rng.integers(-1, nx + 1, 200) + 0.5) / nx).astype(F)      # voxel centres: fractions next to 0 and 1
    po[900:960] = rng.integers(0, 2, (60, 3)).astype(F)                          # the corners
    got = P.sample(vol, po, vertex_centred=bool(convention))
    want = np.array([sc.sample(p) for p in po], F)
    assert np.array_equal(_bits(got), _bits(want))
    if np.dtype(dtype) == np.int8:
        assert (got == -1.0).sum() >= 100 and got.min() == -1.0, "no tap inside the blocks: the clamp is not met"


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_classification_is_the_oracles(ovr, oracle, dtype):
    P = ovr.projection
    vol = SC.volume("random", dtype)
    sc = _scene(oracle, ovr, vol)
    colors, alphas, vr = PC.transfer_function(ovr, "sparse", dtype)
    ct, at = PC.tables(colors, alphas)
    lo, hi = P.normalized_range(vr, dtype)
    assert (lo, hi) == ((F(-1), F(1)) if np.dtype(dtype) == np.int8 else (F(-32768), F(32767)))
    scale = 1.0 if np.dtype(dtype) == np.int8 else 32768.0
    v = (np.concatenate([np.linspace(-1.4, 1.4, 600), np.arange(-15, 16) / 15.0, [0.0, -0.0, -1.0, -128.0 / 127.0, np.nan, np.inf, -np.inf]]) * scale).astype(F)
    got = P.classify(v, ct, at, lo, hi)
    want = np.array([sc.tfn(x) for x in v], F)
    assert np.array_equal(_bits(got[:, 3]), _bits(want[:, 3]))
    assert np.array_equal(_bits(got[:, :3]), _bits(np.clip(want[:, :3], 0, 1)))
    assert (got[:, 3] > 0).any() and (got[:, 3] == 0).any()


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_step_counts_are_the_oracles(ovr, oracle, dtype):
    P = ovr.projection
    for dims in SC.DIMS:
        vol = SC.volume("random", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        for rate in SC.RATES:
            sc = _scene(oracle, ovr, vol, tf="zero", rate=rate)
            r = P.project_rays(vol, org, d, rate, P.MEAN)
            counts = np.array([sc.trace(org[i], d[i])[2].samples for i in range(len(org))])
            assert np.array_equal(r["steps"], counts), (dims, rate)
            assert r["steps"][kind == "through"].max() > 16 and (r["steps"][kind == "miss"] == 0).all()


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_accuracy_against_a_float64_walk(ovr, dtype):
    """tests/test_isosurface_model.py::test_accuracy_against_a_float64_walk on the signed ball, the float64 field being signed_cases.sample64:
    |t* - t_ref| <= step / 25 + 4 ulp(t); rays whose float64 samples change side in another step pair are left out, at most 2 % of the hitting rays"""
    I = ovr.isosurface
    total = left_out = 0
    for dims in SC.DIMS:
        vol = SC.volume("ball", dtype, dims)
        org, d, _ = PC.ray_set(dims)
        for rate in SC.RATES:
            step = 1.0 / rate
            inv, wp = ovr.clipping.volume_constants(dims)
            t0, t1, box = ovr.clipping.world_intervals(org, d, inv, wp)
            tm, count = ovr.projection.steps(t0, t1, F(1) / F(rate), box)
            pos = org.astype(np.float64)[:, None, :] + np.nan_to_num(tm).astype(np.float64)[:, :, None] * d.astype(np.float64)[:, None, :]
            s64 = SC.sample64(vol, (pos / np.array(dims, np.float64)).reshape(-1, 3)).reshape(tm.shape)
            valid = np.arange(tm.shape[1])[None, :] < count[:, None]
            edges = [x for k, x in SC.EDGES[np.dtype(dtype)].items() if k != "all_minimum"]
            for iso in list(SC.scaled(IC.ISOVALUES["ball"], dtype)) + edges:
                r = I.trace_rays(vol, org, d, rate, [iso], shadows=False)
                h = np.flatnonzero(r["hit"])
                cross = np.zeros(tm.shape, bool)
                cross[:, 1:] = ((float(iso) <= s64[:, 1:]) != (float(iso) <= s64[:, :-1])) & valid[:, 1:]
                first64 = np.where(cross.any(1), cross.argmax(1), -1)
                ref = SC.root64(vol, org[h], d[h], r["tm_before"][h], r["tm_at"][h], float(iso))
                same_pair = ~np.isnan(ref) & (first64[h] == r["steps"][h] - 1)
                total += len(h)
                left_out += int((~same_pair).sum())
                t = r["t"][h][same_pair].astype(np.float64)
                err = np.abs(t - ref[same_pair])
                bound = step / 25.0 + 4.0 * np.spacing(r["t"][h][same_pair]).astype(np.float64)
                assert (err <= bound).all(), (dims, rate, float(iso), float(err.max()))
    assert total > 200 and left_out <= 0.02 * total, (left_out, total)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ("ball", "slab", "plateau"))
def test_the_side_assumed_for_a_skipped_cell_by_brute_force(ovr, oracle, kind, dtype):
    """tests/test_isosurface_model.py's brute force over the ORACLE's macrocell ranges of the signed volumes: wherever the walk would drop a fetch, the side it
    assumes is the side of the sample the fetch would have returned - for the model's samples and, for int8, the product's arithmetic - with the type's edge
    isovalues among the levels; `ball` has cells that hold the type's minimum alone"""
    P, I = ovr.projection, ovr.isosurface
    vol = SC.volume(kind, dtype)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    mm, _ = _scene(oracle, ovr, vol).macrocells()
    assert np.array_equal(_bits(mm), _bits(P.macrocell_ranges(vol)))
    lowest = F(-1) if np.dtype(dtype) == np.int8 else F(-32768)
    if kind == "ball":
        assert (mm[..., 1] == lowest).sum() >= 2, "no cell holds the type's minimum alone"
    assert mm[..., 0].min() < 0 < mm[..., 1].max(), "the value range does not straddle zero"
    rng = np.random.default_rng(43)
    po = np.concatenate([_dense_positions(dims, rng), rng.random((40000, 3)).astype(F)])
    c = P.tap_cell(P.tap_coordinates(po, dims)[0], dims)
    lo, hi = mm[c[:, 2], c[:, 1], c[:, 0], 0], mm[c[:, 2], c[:, 1], c[:, 0], 1]
    samplers = [P.sample(vol, po)]
    if I.product_sampler(vol) is not None:
        samplers.append(I.product_sampler(vol)(po))
    tops = np.unique(mm[..., 1])
    levels = list(SC.scaled(IC.ISOVALUES[kind], dtype)) + list(SC.EDGES[np.dtype(dtype)].values())
    levels += [tops[0], np.nextafter(tops[0], F(np.inf)), tops[-1], np.nextafter(tops[-1], F(np.inf)), np.unique(mm[..., 0])[-1]]
    levels = list(np.unique(np.array(levels, F)))
    dropped = 0
    for sets in [[x] for x in levels] + [levels[:4]]:
        iso = I.isovalues(sets)
        fetch, below = I.skipped_side(lo, hi, iso)
        dropped += int((~fetch).sum())
        for s in samplers:
            assert np.array_equal(I.side(s, iso)[~fetch], below[~fetch]), (kind, [float(x) for x in iso])
    assert dropped > 1000


@pytest.mark.parametrize("kind", ("random", "ball", "plateau"))
def test_product_sampler_int8_against_the_per_voxel_tap(ovr, kind):
    """DESIGN.md section 16, with u = 2^-24, W = hi - lo, M = max(|lo|, |hi|) of the normalised voxels: three lerp levels leave each tap within
    3 u (W + M)(1 + 2^-21) of the exact trilinear value of its inputs; normalising once behind the filter adds less than 3 u M; the per-voxel tap's inputs are
    rounded quotients, at most u M off each, which the convex filter passes on.  The two taps therefore differ by less than
    (6 (1 + 2^-21) + 4) u (W + M) < 11 u (W + M) - and both give exactly -1.0 where all eight voxels are -128 or -127"""
    P, I = ovr.projection, ovr.isosurface
    vol = SC.minimum_blocks(np.int8) if kind == "random" else SC.volume(kind, np.int8)
    nz, ny, nx = vol.shape
    rng = np.random.default_rng(47)
    po = np.concatenate([_dense_positions((nx, ny, nz), rng), rng.random((40000, 3)).astype(F)])
    a, b = P.sample(vol, po).astype(np.float64), I.product_sampler(vol)(po).astype(np.float64)
    v = SC.values64(vol)
    W, M = v.max() - v.min(), max(abs(v.min()), abs(v.max()))
    d = np.abs(a - b)
    print(f"{kind}: max |product - per-voxel| {d.max():.3g}, bound {11 * U * (W + M):.3g}; {int((d > 0).sum())} of {len(d)} taps differ")
    assert d.max() < 11 * U * (W + M)
    assert np.array_equal(a == -1.0, b == -1.0) and a.min() >= -1.0 and b.min() >= -1.0, "a tap below -1: the clamp is missing"
    if kind != "plateau":      # (the lowest plateau is 37 / 255 of full scale: no voxel at the minimum)
        assert (a == -1.0).sum() > 100


# ---- 2. the conditions that keep the GPU tests discriminating ---------------------------------------------------------------------------------------

def _clamp_case(ovr):
    dims = SC.DIMS[0]
    vol = SC.volume("ball", np.int8, dims)
    org, d, _ = PC.ray_set(dims)
    return vol, org, d, SC.clamp_isovalues()


def test_a_tap_without_the_clamp_changes_the_crossings(ovr):
    """int8 `ball` at (40, 33, 18), rate 1, the isovalues of signed_cases.clamp_isovalues: more than 40 of the 100 rays hit, and a tap that normalises -128 to
    -128 / 127 instead of -1 moves t* on at least a quarter of the rays (the exterior of the ball is -128: every first crossing starts there)"""
    I = ovr.isosurface
    vol, org, d, iso = _clamp_case(ovr)
    assert len(org) == 100 and (vol == -128).sum() > 1000
    mutant = (vol.astype(F) / F(127)).astype(F)      # a float volume: what a tap without the clamp filters
    for sampler in (None, I.product_sampler(vol)):
        want = I.trace_rays(vol, org, d, 1.0, iso, shadows=False, sampler=sampler)
        got = I.trace_rays(mutant, org, d, 1.0, iso, shadows=False)
        changed = (want["hit"] != got["hit"]) | (_bits(want["t"]) != _bits(got["t"]))
        print(f"{int(want['hit'].sum())} rays hit; without the clamp {int(changed.sum())} rays change")
        assert want["hit"].sum() > 40 and changed.sum() >= 25


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_a_tap_that_reads_unsigned_changes_the_hit_mask(ovr, dtype):
    I = ovr.isosurface
    dims = SC.DIMS[0]
    vol = SC.volume("ball", dtype, dims)
    org, d, _ = PC.ray_set(dims)
    iso = SC.scaled(IC.NESTED["ball"][1:3], dtype)
    want = I.trace_rays(vol, org, d, 1.0, iso, shadows=False)
    got = I.trace_rays(vol.view(SC.UNSIGNED[np.dtype(dtype)]), org, d, 1.0, iso, shadows=False)
    changed = want["hit"] != got["hit"]
    print(f"{np.dtype(dtype).name}: {int(want['hit'].sum())} rays hit; read as unsigned {int(changed.sum())} hit flags change")
    assert changed.sum() >= 25
    # the projections see it too: the extrema move on most rays
    P = ovr.projection
    rnd = SC.volume("random", dtype, dims)
    a, b = P.project_rays(rnd, org, d, 1.0, P.MAXIMUM), P.project_rays(rnd.view(SC.UNSIGNED[np.dtype(dtype)]), org, d, 1.0, P.MAXIMUM)
    assert (_bits(a["v"]) != _bits(b["v"])).sum() >= 50


@pytest.mark.parametrize("kind", ("ball", "random"))
def test_the_all_minimum_isovalue_gives_no_hit(ovr, kind):
    """-1.0 exactly: every int8 sample is on or above it (the clamp), so no ray changes side - without the clamp the exterior's samples lie below it"""
    I = ovr.isosurface
    for dims in SC.DIMS:
        vol = SC.minimum_blocks(np.int8, dims) if kind == "random" else SC.volume("ball", np.int8, dims)
        org, d, _ = PC.ray_set(dims)
        for rate in SC.RATES:
            for sampler in (None, I.product_sampler(vol)):
                for skipping in (False, True):
                    r = I.trace_rays(vol, org, d, rate, [SC.INT8_EDGES["all_minimum"]], shadows=False, sampler=sampler, skipping=skipping)
                    assert not r["hit"].any(), (dims, rate, skipping)
    mutant = (SC.volume("ball", np.int8).astype(F) / F(127)).astype(F)
    org, d, _ = PC.ray_set(SC.DIMS[0])
    assert I.trace_rays(mutant, org, d, 1.0, [F(-1.0)], shadows=False)["hit"].sum() > 40


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_every_gpu_frame_case_has_enough_to_compare(ovr, oracle, dtype):
    """more than 40 hit pixels in every isosurface frame case of signed_cases.ISO_FRAMES, more than 100 marched pixels in the projection frames"""
    I, P = ovr.isosurface, ovr.projection
    w, h = SC.SIZE
    basis = oracle.camera_basis(*SC.CAMERAS[SC.CAMERA], SC.FOVY, w, h).reshape(4, 3)
    dirs = P.pixel_rays(basis, w, h, None).reshape(-1, 3)
    org = np.broadcast_to(basis[0], dirs.shape)
    for name, (kind, iso, opacities) in SC.iso_frames(dtype).items():
        vol = SC.volume(kind, dtype)
        r = I.trace_rays(vol, org, dirs, SC.FRAME_RATE, iso, shadows=False, sampler=I.product_sampler(vol), opacities=opacities)
        hits = int((r["n_events"] > 0).sum()) if opacities is not None else int(r["hit"].sum())
        print(f"{np.dtype(dtype).name} {name}: {hits} hit pixels")
        assert hits > 40, (name, hits)
    for kind in SC.PROJECTION_KINDS:
        hi, lo = (P.project_rays(SC.volume(kind, dtype), org, dirs, SC.FRAME_RATE, mode) for mode in (P.MAXIMUM, P.MINIMUM))
        assert hi["marched"].sum() > 100 and (hi["v"][hi["marched"]] > 0).any() and (lo["v"][lo["marched"]] < 0).any(), kind
