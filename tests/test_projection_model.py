"""The projection model (open-volume-renderer_amd/projection.py, include/ovr_hip.h ovr_hip_set_projection) on the CPU, pinned against the UNMODIFIED oracle: its
intervals are oracle.intersect_box's, its samples OracleScene.sample's bit for bit (f32, u16, u8), its classification OracleScene.tfn's, its step count the
`samples` counter of trace() under an all-zero alpha table; the threshold identity against the oracle's frame; and the range-skipping slack by brute force over
the oracle's macrocell ranges.  No GPU."""
import os
import re

import numpy as np
import pytest

import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ["ovr_hip_set_projection", "ovr_hip_get_projection", "ovr_hip_project_floats"]


@pytest.fixture(scope="module")
def P(ovr):
    return ovr.projection


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _scene(oracle, ovr, vol, tf="sparse", rate=1.0, cam="oblique", shading=0, convention=0):
    colors, alphas, vr = PC.transfer_function(ovr, tf, vol.dtype)
    return oracle.OracleScene(vol, colors, alphas, vr, PC.CAMERAS[cam], PC.SIZE[0], PC.SIZE[1], fovy=PC.FOVY, rate=rate, shading=shading, convention=convention)


def test_entry_points_are_declared_bound_and_exported(ovr):
    hdr = open(os.path.join(ROOT, "include", "ovr_hip.h")).read()
    lib = ovr._lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in ovr._lib.SYMBOLS and hasattr(lib, name), name
    assert (ovr.PROJECT_OFF, ovr.PROJECT_MAXIMUM, ovr.PROJECT_MINIMUM, ovr.PROJECT_MEAN) == (0, 1, 2, 3)
    for k, name in enumerate(("OFF", "MAXIMUM", "MINIMUM", "MEAN")):
        assert re.search(r"#define OVR_HIP_PROJECT_%s %d\b" % (name, k), hdr)
    assert lib.ovr_hip_set_projection(None, 1) < 0 and lib.ovr_hip_get_projection(None, None) < 0 and lib.ovr_hip_project_floats(None, None, None, None, 0, 1, 0) < 0


@pytest.mark.parametrize("dims", PC.DIMS, ids=str)
def test_intervals_and_step_counts_are_the_oracles(P, ovr, oracle, dims):
    """the interval of every ray of the set is oracle.intersect_box's, and the number of steps is what the oracle's march counts when nothing ends it early"""
    vol = PC.volume("random", np.float32, dims)
    org, d, kind = PC.ray_set(dims)
    inv, wp = ovr.clipping.volume_constants(dims)
    oo, od = ovr.clipping.to_object(org, inv, wp), (d * inv).astype(F)
    t0, t1, hit = ovr.clipping.intersect(oo, od)
    want = [oracle.intersect_box(oo[i], od[i]) for i in range(len(org))]
    assert np.array_equal(hit, [w[0] for w in want])
    assert np.array_equal(_bits(t0)[hit], _bits([w[1] for w in want])[hit]) and np.array_equal(_bits(t1)[hit], _bits([w[2] for w in want])[hit])
    assert not hit[kind == "miss"].any() and hit[kind != "miss"].all()
    for rate in PC.RATES:
        sc = _scene(oracle, ovr, vol, tf="zero", rate=rate)
        r = P.project_rays(vol, org, d, rate, P.MAXIMUM)
        counts = np.array([sc.trace(org[i], d[i])[2].samples for i in range(len(org))])
        assert np.array_equal(r["steps"], counts), rate
        if rate == 1.0:
            assert 0 < r["steps"][kind == "grazer"].max() < 4 and r["steps"][kind == "through"].max() > 16


@pytest.mark.parametrize("convention", (0, 1), ids=("cell", "vertex"))
@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_samples_are_the_oracles_bit_for_bit(P, ovr, oracle, dtype, convention):
    vol = PC.volume("random", dtype)
    sc = _scene(oracle, ovr, vol, convention=convention)
    rng = np.random.default_rng(21)
    po = (rng.random((1500, 3)) * 1.1 - 0.05).astype(F)
    nx = vol.shape[2]
    po[:200, 0] = ((rng.integers(-1, nx + 1, 200) + 0.5) / nx).astype(F)   # voxel centres: fractions next to 0 and 1
    po[200:260] = rng.integers(0, 2, (60, 3)).astype(F)                    # the corners
    got = P.sample(vol, po, vertex_centred=bool(convention))
    want = np.array([sc.sample(p) for p in po], F)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_classification_is_the_oracles(P, ovr, oracle, dtype):
    vol = PC.volume("random", dtype)
    sc = _scene(oracle, ovr, vol)
    colors, alphas, vr = PC.transfer_function(ovr, "sparse", dtype)
    ct, at = PC.tables(colors, alphas)
    lo, hi = P.normalized_range(vr, dtype)
    scale = {np.dtype(np.float32): 1.0, np.dtype(np.uint16): 65535.0, np.dtype(np.uint8): 1.0}[np.dtype(dtype)]
    v = (np.concatenate([np.linspace(-0.7, 1.2, 400), np.arange(16) / 15.0, [np.nan, np.inf, -np.inf]]) * scale).astype(F)
    got = P.classify(v, ct, at, lo, hi)
    want = np.array([sc.tfn(x) for x in v], F)
    assert np.array_equal(_bits(got[:, 3]), _bits(want[:, 3]))
    assert np.array_equal(_bits(got[:, :3]), _bits(np.clip(want[:, :3], 0, 1)))
    assert (got[:, 3] > 0).any() and (got[:, 3] == 0).any()


def test_reductions_follow_the_definition(P):
    s = np.array([[1.0, 3.0, np.nan, 3.0, -0.0, 0.0, 2.0], [np.nan] * 7, [-np.inf, 5.0, 5.0, 1.0, 1.0, 9.0, 9.0]], F)
    tm = np.tile(np.arange(1, 8, dtype=F), (3, 1))
    count = np.array([7, 7, 5])
    v, t = P.reduce(s, tm, count, P.MAXIMUM)
    assert list(v) == [3.0, -np.inf, 5.0] and list(t) == [2.0, 0.0, 2.0]            # the first of equal samples; a NaN is never selected
    v, t = P.reduce(s, tm, count, P.MINIMUM)
    assert list(v[[0, 2]]) == [0.0, -np.inf] and np.signbit(v[0]) and list(t) == [5.0, 0.0, 1.0] and v[1] == np.inf
    big = np.array([[1e8, 1.0, -1e8, 1.0, 1.0, 1.0, 1.0, 1.0, 3.0]], F)
    v, t = P.reduce(big, np.zeros_like(big), np.array([9]), P.MEAN)
    a = [F(F(F(1e8) + F(1)) + F(3)), F(F(1) + F(1)), F(F(-1e8) + F(1)), F(F(1) + F(1))]   # four interleaved sums
    assert v[0] == F(F(F(a[0] + a[1]) + F(a[2] + a[3])) / F(9)) and t[0] == 0


@pytest.fixture(scope="module")
def threshold_inputs(ovr, oracle):
    """the threshold identity's fixed inputs (the GPU test uses the same): the smooth volume under the monotone `sparse` table at both rates and cameras"""
    out = {}
    for dtype in (np.float32, np.uint8):
        vol = PC.volume("smooth", dtype)
        for cam in PC.CAMERAS:
            for rate in PC.RATES:
                sc = _scene(oracle, ovr, vol, tf="sparse", rate=rate, cam=cam)
                out[(np.dtype(dtype).name, cam, rate)] = (vol, sc.render(), sc)
    return out


def test_threshold_identity_against_the_oracles_frame(P, ovr, oracle, threshold_inputs):
    """a monotone non-decreasing alpha table: the oracle's march finds alpha > 0 exactly where the maximum's classification does"""
    for (dname, cam, rate), (vol, (ref, _, cnt), sc) in threshold_inputs.items():
        assert cnt.borderline_samples == 0, "the precondition: no sample whose corrected opacity rounds towards 0"
        colors, alphas, vr = PC.transfer_function(ovr, "sparse", vol.dtype)
        ct, at = PC.tables(colors, alphas)
        assert (np.diff(at) >= 0).all()
        basis = oracle.camera_basis(*PC.CAMERAS[cam], PC.FOVY, *PC.SIZE).reshape(4, 3)
        rgba, layer, c = P.frame(vol, basis, PC.SIZE, rate, P.MAXIMUM, ct, at, P.normalized_range(vr, vol.dtype))
        assert np.array_equal(rgba[..., 3] > 0, ref[..., 3] > 0), (dname, cam, rate)
        assert 40 < (rgba[..., 3] > 0).sum() < rgba[..., 3].size - 40
        assert c["rays"] == cnt.rays


def _dense_positions(dims, rng):
    """object positions whose voxel coordinates have fractions at and next to 0 and 1, on every axis, through every macrocell border"""
    per_axis = []
    for n in dims:
        i = np.concatenate([rng.integers(-1, n, 10), [-1, 0, 14, 15, 16, n - 2, n - 1]]).astype(np.float64)
        f = np.array([0.0, 2.0 ** -24, 2.0 ** -12, 0.25, 0.5, 1 - 2.0 ** -12, 1 - 2.0 ** -23])
        x = (i[:, None] + f[None, :]).ravel()
        per_axis.append(((x + 0.5) / n).astype(F))
    k = [rng.integers(0, len(a), 60000) for a in per_axis]
    return np.stack([per_axis[a][k[a]] for a in range(3)], 1)


@pytest.mark.parametrize("kind,dtype", [("random", np.float32), ("random", np.uint16), ("random", np.uint8), ("plateau", np.uint8), ("plateau", np.float32),
                                        ("slab", np.float32), ("twin", np.uint8)], ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_slack_covers_every_sample_and_skipping_changes_nothing(P, ovr, oracle, kind, dtype):
    """brute force: every sample lies within [lo - slack, hi + slack] of the ORACLE's range of its tap_cell, and the model's skipping reduction equals its plain
    one, tm* included.  With voxels normalised one by one (f32, u16, and u8 as the oracle and the exact-parity build sample it) no sample leaves [lo, hi] itself -
    a tap's fraction is at most 1 - 2^-24, so no lerp level can pass its larger input - and this part would hold with a slack of 0.  Where the slack is NEEDED
    is the product's 8-bit arithmetic, which normalises once behind the filter: on the plateau volume thousands of its samples exceed their cell's stored
    maximum by an ulp, which is asserted"""
    vol = PC.volume(kind, dtype)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    mm, _ = _scene(oracle, ovr, vol).macrocells()
    assert np.array_equal(_bits(mm), _bits(P.macrocell_ranges(vol)))
    rng = np.random.default_rng(31)
    po = np.concatenate([_dense_positions(dims, rng), rng.random((40000, 3)).astype(F)])
    s = P.sample(vol, po)
    i0, _ = P.tap_coordinates(po, dims)
    c = P.tap_cell(i0, dims)
    lo, hi = mm[c[:, 2], c[:, 1], c[:, 0], 0], mm[c[:, 2], c[:, 1], c[:, 0], 1]
    sl = P.slack(lo, hi)
    assert (sl > 0).all() and (s >= lo - sl).all() and (s <= hi + sl).all()
    outside = int(((s < lo) | (s > hi)).sum())
    print(f"{kind} {np.dtype(dtype).name}: {outside} of {len(s)} samples lie outside their cell's range (by at most {float(np.maximum(lo - s, s - hi).max()):.3g}; slack >= {float(sl.min()):.3g})")
    # the product normalises 8-bit voxels behind the filter: its samples obey the same bound
    if np.dtype(dtype) == np.uint8:
        raw = P.sample(vol.astype(F), po)
        sp = (raw * F(F(1) / F(255))).astype(F)
        assert (sp >= lo - sl).all() and (sp <= hi + sl).all()
        beyond = int(((sp < lo) | (sp > hi)).sum())
        print(f"{kind} uint8, normalised behind the filter: {beyond} of {len(sp)} samples lie outside their cell's range (by at most {float(np.maximum(lo - sp, sp - hi).max()):.3g})")
        if kind == "plateau":
            assert beyond > 1000, "the slack is not idle: without it these samples' cells would be skipped wrongly"
    org, d, _ = PC.ray_set(dims)
    for rate in PC.RATES:
        for mode in (P.MAXIMUM, P.MINIMUM):
            a = P.project_rays(vol, org, d, rate, mode)
            b = P.project_rays(vol, org, d, rate, mode, skipping=True)
            assert np.array_equal(_bits(a["v"]), _bits(b["v"])) and np.array_equal(_bits(a["tm"]), _bits(b["tm"])) and np.array_equal(a["steps"], b["steps"])
            assert (b["fetched"] <= b["steps"]).all()
            if kind in ("slab", "plateau") and mode == P.MAXIMUM:   # (twin: a cell that holds the bound itself proves nothing)
                assert b["fetched"].sum() < b["steps"].sum(), "nothing was skipped"


def test_a_tie_keeps_the_first_sample_under_skipping(P):
    """the same maximum twice along the ray: the later sample is fetched (its cell's range, widened by the slack, does not prove it smaller) and does not replace
    the first - tm* stays; a cell whose widened range ends below the bound is skipped from the next round on"""
    s = np.full((1, 40), 0.25, F)
    s[0, 3] = s[0, 30] = 0.75
    tm = np.arange(40, dtype=F)[None, :]
    lo, hi = np.full((1, 40), 0.25, F), np.full((1, 40), 0.75, F)
    v, t, fetched = P.reduce_skipping(s, tm, np.array([40]), lo, hi, P.MAXIMUM)
    assert v[0] == 0.75 and t[0] == 3.0 and fetched[0] == 40
    hi[0, 20:] = 0.7
    s[0, 30] = 0.7
    v, t, fetched = P.reduce_skipping(s, tm, np.array([40]), lo, hi, P.MAXIMUM)
    assert v[0] == 0.75 and t[0] == 3.0 and fetched[0] == 20
