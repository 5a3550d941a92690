"""The translucent isosurfaces of the model (open-volume-renderer_amd/isosurface.py, include/ovr_hip.h ovr_hip_set_isosurface_layers) on the
CPU: all-ones opacities are the opaque model bit for bit, the order of a step's events, the composite against the closed form, saturation, t* of every event
against a float64 walk, the partial shadow of one shell, and the skipping walk against the plain one.  No GPU."""
import os
import re

import numpy as np
import pytest

import isosurface_cases as IC
import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ["ovr_hip_set_isosurface_layers", "ovr_hip_get_isosurface_layers", "ovr_hip_isosurface_layers_floats"]
CLOSE_PAIR, CLOSE_FOUR = (0.40, 0.43), (0.40, 0.41, 0.42, 0.43)
RAY_KEYS = ("hit", "k", "iso", "t", "steps", "fetched", "normal", "shadow", "pos", "shadow_steps", "shadow_fetched", "tm_before", "tm_at")


@pytest.fixture(scope="module")
def I(ovr):
    return ovr.isosurface


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _camera_rays(ovr, oracle, cam):
    w, h = IC.SIZE
    basis = oracle.camera_basis(*IC.CAMERAS[cam], IC.FOVY, w, h).reshape(4, 3)
    d = ovr.projection.pixel_rays(basis, w, h, None).reshape(-1, 3)
    return basis, np.broadcast_to(np.asarray(basis[0], F), d.shape), d


def test_entry_points_are_declared_bound_and_exported(ovr):
    hdr = open(os.path.join(ROOT, "include", "ovr_hip.h")).read()
    lib = ovr._lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in ovr._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct ovr_hip_isosurface_layers \{", hdr)
    assert lib.ovr_hip_set_isosurface_layers(None, None, None, 0) < 0 and lib.ovr_hip_get_isosurface_layers(None, None) < 0
    assert lib.ovr_hip_isosurface_layers_floats(None, None, None, None, 0, 8, 0) < 0


def test_the_opacities_travel_with_their_isovalues(I):
    assert list(I.opacities_of([0.5, 1.0, 0.25], [0.7, 0.2, 0.5])) == [F(1.0), F(0.25), F(0.5)]
    for bad in ([0.0, 0.5], [0.5, 1.5], [0.5, np.nan], [0.5, -0.1], [0.5], [0.5, np.inf]):
        with pytest.raises(ValueError):
            I.opacities_of(bad, [0.1, 0.2])
    assert [list(I.events_of_step(a, b)) for a, b in ((0, 1), (1, 4), (4, 1), (2, 0), (3, 2))] == [[0], [1, 2, 3], [3, 2, 1], [1, 0], [2]]


@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", IC.KINDS)
def test_all_ones_is_the_opaque_model(I, ovr, oracle, kind, dtype):
    """opacities=None against all-ones: the bits of every output of trace_rays and frame"""
    vol = IC.volume(kind, dtype)
    iso = IC.scaled(IC.ISOVALUES[kind], dtype)
    ones = np.ones(len(iso), F)
    org, d, _ = PC.ray_set(IC.DIMS[0])
    for skipping in (False, True):
        a = I.trace_rays(vol, org, d, 2.5, iso, light=(0.3, 0.8, -0.52), skipping=skipping)
        b = I.trace_rays(vol, org, d, 2.5, iso, light=(0.3, 0.8, -0.52), skipping=skipping, opacities=ones)
        assert a["hit"].sum() > 10
        for name in RAY_KEYS:
            assert a[name].dtype == b[name].dtype and np.array_equal(a[name].view(np.uint32) if a[name].dtype == F else a[name], b[name].view(np.uint32) if b[name].dtype == F else b[name]), (kind, name)
        assert np.array_equal(b["n_events"], a["hit"].astype(np.int64)) and (b["A"][a["hit"]] == 1).all() and not b["A"][~a["hit"]].any()
    colors, alphas, vr = PC.transfer_function(ovr, "sparse", vol.dtype)
    ct, _ = PC.tables(colors, alphas)
    basis = oracle.camera_basis(*IC.CAMERAS["oblique"], IC.FOVY, *IC.SIZE).reshape(4, 3)
    for shading in (I.NONE, I.FULL):
        fa = I.frame(vol, basis, IC.SIZE, 1.0, iso, ct, ovr.projection.normalized_range(vr, vol.dtype), shading=shading)
        fb = I.frame(vol, basis, IC.SIZE, 1.0, iso, ct, ovr.projection.normalized_range(vr, vol.dtype), shading=shading, opacities=ones)
        assert np.array_equal(_bits(fa[0]), _bits(fb[0])) and np.array_equal(_bits(fa[1]), _bits(fb[1])) and fa[2] == fb[2], (kind, shading)


def test_event_order(I, ovr, oracle):
    """a ray through the ball's centre meets the nested shells as 0, 1, 2, 3, 3, 2, 1, 0; a step that crosses two close levels lists them ascending while the
    samples rise and descending while they fall"""
    vol = IC.volume("ball", np.float32)
    nested = IC.scaled(IC.NESTED["ball"], np.float32)
    r = I.trace_rays(vol, [(-30.0, 16.5, 9.0)], [(1.0, 0.0, 0.0)], 1.0, nested, opacities=(0.3,) * 4, shadows=False)
    assert [e["k"] for e in r["events"][0]] == [0, 1, 2, 3, 3, 2, 1, 0]
    ts = [float(e["t"]) for e in r["events"][0]]
    assert ts == sorted(ts) and r["steps"][0] == 40      # the ray never saturates (A = 1 - 0.7^8): it walks all its steps
    pair = IC.scaled(CLOSE_PAIR, np.float32)
    double = 0
    for cam in sorted(IC.CAMERAS):
        _, org, d = _camera_rays(ovr, oracle, cam)
        r = I.trace_rays(vol, org, d, 1.0, pair, opacities=(0.3, 0.3), shadows=False)
        for row in r["events"]:
            steps = [e["i"] for e in row]
            assert steps == sorted(steps)
            for i in set(steps):
                ks = [e["k"] for e in row if e["i"] == i]
                if len(ks) == 2:
                    double += 1
                    first_half = row[0]["i"] == i                                             # into the ball the samples rise, out of it they fall
                    assert ks == ([0, 1] if first_half else [1, 0]), (cam, row)
                    a, b = [e["t"] for e in row if e["i"] == i]
                    assert a <= b                                                             # the order the ray meets them
    assert double >= 20, double


def test_constant_opacity_is_the_closed_form(I, ovr, oracle):
    """m events of one opacity a: A = 1 - (1 - a)^m, the recurrence's m fused operations each within half an ulp of a value below 1: within m ulp"""
    vol = IC.volume("ball", np.float32)
    _, org, d = _camera_rays(ovr, oracle, "oblique")
    seen = set()
    for a in (0.3, 0.05, 0.6):
        r = I.trace_rays(vol, org, d, 1.0, IC.scaled(IC.NESTED["ball"], np.float32), opacities=(a,) * 4, shadows=False)
        for row in r["events"]:
            for m, e in enumerate(row, 1):
                want = 1.0 - (1.0 - float(F(a))) ** m
                assert abs(float(e["A"]) - want) <= m * float(np.spacing(F(want))), (a, m, float(e["A"]), want)
                seen.add(m)
        assert np.array_equal(r["A"][r["hit"]], np.array([row[-1]["A"] for row in r["events"] if row], F))
    assert max(seen) >= 6


def test_saturation_ends_the_ray(I, ovr, oracle):
    """four close levels at opacity 0.9: A reaches 0.9999f at the fourth event, the ray ends inside the step that holds it"""
    vol = IC.volume("ball", np.float32)
    four = IC.scaled(CLOSE_FOUR, np.float32)
    hits = 0
    for cam in sorted(IC.CAMERAS):
        _, org, d = _camera_rays(ovr, oracle, cam)
        n = I.trace_rays(vol, org, d, 1.0, [F(1e9)], shadows=False)["steps"]          # a miss walks every step
        r = I.trace_rays(vol, org, d, 1.0, four, opacities=(0.9,) * 4, shadows=False)
        h = r["hit"]
        assert (r["n_events"][h] == 4).all() and (r["steps"][h] < n[h]).all() and np.array_equal(r["steps"][~h], n[~h])
        assert (r["A"][h] >= I.SATURATED).all() and all(row[2]["A"] < I.SATURATED for row in r["events"] if row)
        assert np.array_equal(r["steps"][h], np.array([row[-1]["i"] + 1 for row in r["events"] if row]))
        hits += int(h.sum())
        mixed = I.trace_rays(vol, org, d, 1.0, IC.scaled(IC.NESTED["ball"], np.float32), opacities=(0.3, 0.4, 0.5, 1), shadows=False)
        early = mixed["hit"] & (mixed["steps"] < n)
        assert early.sum() >= 10 and (mixed["A"][early] == 1).all() and (mixed["n_events"] >= 4).sum() >= 40
    assert hits >= 60


@pytest.mark.parametrize("kind", ("smooth", "ball"))
def test_accuracy_of_every_event_against_a_float64_walk(I, ovr, oracle, kind):
    """section 17's bound for every event: |t* - t_ref| <= step / 25 + 4 ulp(t), t_ref the float64 root of the same bracket.  Left out: events whose float64
    samples do not bracket the level in the model's step pair (samples within rounding of the level); at most 2 %, asserted"""
    vol = IC.volume(kind, np.float32)
    iso = IC.scaled(IC.NESTED[kind], np.float32)
    total = left_out = 0
    for cam in sorted(IC.CAMERAS):
        _, org, d = _camera_rays(ovr, oracle, cam)
        for rate in IC.RATES:
            step = 1.0 / rate
            f = I.trace_rays(vol, org, d, rate, iso, opacities=(0.3,) * 4, shadows=False)["flat"]
            ref = np.concatenate([IC.root64(vol, org[f["ray"]][f["k"] == k], d[f["ray"]][f["k"] == k], f["tm_before"][f["k"] == k], f["tm_at"][f["k"] == k], float(iso[k]))
                                  for k in range(4)])
            t = np.concatenate([f["t"][f["k"] == k] for k in range(4)])
            ok = ~np.isnan(ref)
            err = np.abs(t[ok].astype(np.float64) - ref[ok])
            bound = step / 25.0 + 4.0 * np.spacing(t[ok]).astype(np.float64)
            print(f"{kind} {cam} rate {rate}: {len(t)} events, {int((~ok).sum())} left out, max error {err.max() / step:.3g} step (bound {1 / 25:.3g})")
            assert (err <= bound).all(), (kind, cam, rate, float(err.max()))
            assert (f["tm_before"] <= f["t"]).all() and (f["t"] <= f["tm_at"]).all()
            total += len(t)
            left_out += int((~ok).sum())
    assert total > 1000 and left_out <= 0.02 * total, (left_out, total)


def test_partial_shadow_of_one_shell(I):
    """a floor under a ball, one level of opacity 0.5, the light straight above: the floor behind the ball sees the light's ray pass into the ball and out of it -
    0.5 + 0.5 * 0.5 = 0.75 -, the floor beside it sees nothing, 0; the ball's own far side sees one crossing, 0.5, its near side none"""
    n = 32
    z, y, x = np.meshgrid(np.arange(n) + 0.5, np.arange(n) + 0.5, np.arange(n) + 0.5, indexing="ij")
    ball = np.clip(1.0 - np.sqrt((x - 16.0) ** 2 + (y - 18.0) ** 2 + (z - 16.0) ** 2) / 10.0, 0.0, 1.0)      # the level 0.4: a sphere of radius 6 around y = 18
    floor = np.clip((4.0 - y) / 4.0, 0.0, 1.0)                                                                # the level 0.4: the plane y = 2.4
    vol = np.maximum(ball, floor).astype(F)
    gx, gz = np.meshgrid(np.arange(4.25, 28.0, 0.5), np.arange(4.25, 28.0, 0.5))
    org = np.stack([gx.ravel(), np.full(gx.size, 40.0), gz.ravel()], 1).astype(F)
    d = np.broadcast_to(np.array([0.0, -1.0, 0.0], F), org.shape)
    rho = np.hypot(org[:, 0] - 16.0, org[:, 2] - 16.0)
    for rate in IC.RATES:
        r = I.trace_rays(vol, org, d, rate, [F(0.4)], opacities=[0.5], light=(0.0, 1.0, 0.0))
        through, beside = rho < 4.5, rho > 7.5          # (in between the chord is too short for the shadow ray's samples, or the ray grazes)
        assert through.sum() > 100 and beside.sum() > 1000
        assert (r["n_events"][through] == 3).all() and (r["n_events"][beside] == 1).all()
        for row in (r["events"][j] for j in np.flatnonzero(through)):
            assert [float(e["shadow"]) for e in row] == [0.0, 0.5, 0.75], row
            assert [float(e["A"]) for e in row] == [0.5, 0.75, 0.875]
        for row in (r["events"][j] for j in np.flatnonzero(beside)):
            assert float(row[0]["shadow"]) == 0.0 and abs(float(row[0]["t"]) - 37.6) < 0.05


@pytest.mark.parametrize("kind,dtype", [("ball", np.float32), ("plateau", np.uint8), ("slab", np.float32), ("smooth", np.uint16)], ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_skipping_changes_nothing(I, ovr, kind, dtype):
    """the skipping walk against the plain one, bit for bit - also with an isovalue AT a cell's maximum and one ulp above it, as section 17's test does"""
    vol = IC.volume(kind, dtype)
    tops = np.unique(ovr.projection.macrocell_ranges(vol)[..., 1])
    base = IC.scaled(IC.NESTED.get(kind, IC.ISOVALUES[kind]), dtype)
    skipped = 0
    org, d, _ = PC.ray_set(IC.DIMS[0])
    for iso in (base, np.unique(np.concatenate([base[:2], [tops[0], np.nextafter(tops[0], F(np.inf))]]).astype(F)),
                np.unique(np.concatenate([base[:2], [tops[-1], np.nextafter(tops[-1], F(np.inf))]]).astype(F))):
        op = np.linspace(0.3, 0.6, len(iso)).astype(F)
        for rate in IC.RATES:
            a = I.trace_rays(vol, org, d, rate, iso, opacities=op, light=(0.3, 0.8, -0.52))
            b = I.trace_rays(vol, org, d, rate, iso, opacities=op, light=(0.3, 0.8, -0.52), skipping=True)
            for name in ("hit", "k", "steps", "shadow_steps", "n_events"):
                assert np.array_equal(a[name], b[name]), (kind, rate, name)
            for name in ("iso", "t", "normal", "shadow", "A"):
                assert np.array_equal(_bits(a[name]), _bits(b[name])), (kind, rate, name)
            for name in ("ray", "i", "k"):
                assert np.array_equal(a["flat"][name], b["flat"][name]), (kind, rate, name)
            for name in ("t", "normal", "shadow", "A"):
                assert np.array_equal(_bits(a["flat"][name]), _bits(b["flat"][name])), (kind, rate, name)
            assert np.array_equal(a["fetched"], a["steps"]) and (b["fetched"] <= b["steps"]).all() and (b["shadow_fetched"] <= b["shadow_steps"]).all()
            skipped += int((b["steps"] - b["fetched"]).sum())
    assert skipped > 0, "nothing was skipped"
