"""Ambient occlusion of the isosurface model (open-volume-renderer_amd/isosurface.py, include/ovr_hip.h ovr_hip_set_ambient_occlusion) on the
CPU: the direction table and the rotation index, the neutral element (a plane occludes nothing: the K = 0 frame bit for bit), the cavity (everything occludes:
O = 1 exactly), monotony in the radius, the translucent shells against the closed form, and the skipping walk against the plain one.  No GPU."""
import os
import re

import numpy as np
import pytest

import ambient_occlusion_cases as AC
import isosurface_cases as IC
import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = AC.INF
NEW_SYMBOLS = ["ovr_hip_set_ambient_occlusion", "ovr_hip_get_ambient_occlusion", "ovr_hip_get_ambient_occlusion_directions", "ovr_hip_isosurface_ao_floats"]


@pytest.fixture(scope="module")
def I(ovr):
    return ovr.isosurface


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _ulps(a, b):
    """the distance of two arrays of finite float32 of one sign in units in the last place"""
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


def _frame(I, ovr, oracle, vol, cam, iso, ao=None, shading=2, material=None, opacities=None, skipping=False, size=AC.SIZE, rate=1.0):
    colors, alphas, vr = PC.transfer_function(ovr, "unit", vol.dtype)
    ct, _ = PC.tables(colors, alphas)
    basis = oracle.camera_basis(*cam, AC.FOVY, *size).reshape(4, 3)
    kw = {} if material is None else dict(material=material)
    return I.frame(vol, basis, size, rate, iso, ct, ovr.projection.normalized_range(vr, vol.dtype), shading=shading, opacities=opacities, skipping=skipping, ao=ao, **kw)


def _cavity_events(I, K, R, opacities=None, iso=None, skipping=False, rotation=None):
    org, d = AC.cavity_rays()
    rot = np.arange(len(org)) & 15 if rotation is None else np.full(len(org), rotation)
    iso = [AC.level(AC.CAVITY_RADIUS)] if iso is None else iso
    return I.trace_rays(AC.cavity(), org, d, 1.0, iso, opacities=opacities, skipping=skipping, ao=(I.ao_directions(K), R, rot))


def test_entry_points_are_declared_bound_and_exported(ovr):
    hdr = open(os.path.join(ROOT, "include", "ovr_hip.h")).read()
    lib = ovr._lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in ovr._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct ovr_hip_ambient_occlusion \{", hdr)
    assert lib.ovr_hip_set_ambient_occlusion(None, 4, 1.0) < 0 and lib.ovr_hip_get_ambient_occlusion(None, None) < 0
    assert lib.ovr_hip_get_ambient_occlusion_directions(None, None, 0) < 0 and lib.ovr_hip_isosurface_ao_floats(None, None, None, None, 0, 8, 0, 0) < 0


@pytest.mark.parametrize("K", range(1, 17))
def test_direction_table(I, K):
    D = I.ao_directions(K)
    assert D.shape == (16, K, 3) and D.dtype == F
    d64 = D.astype(np.float64)
    # unit length within 2 ulp of 1 (each component was rounded once)
    assert (np.abs(np.sqrt((d64 ** 2).sum(-1)) - 1.0) <= 2 * 2.0 ** -24).all()
    assert (D[..., 2] > 0).all()
    z = np.sqrt(1.0 - (np.arange(K) + 0.5) / K).astype(F)
    assert np.array_equal(_bits(D[..., 2]), _bits(np.broadcast_to(z, (16, K))))
    # the sixteen rotations of an entry differ in azimuth alone: the same radius, the azimuth advancing by 2 pi / 16
    rad = np.hypot(d64[..., 0], d64[..., 1])
    assert (np.abs(rad - np.sqrt((np.arange(K) + 0.5) / K)[None, :]) <= 2.0 ** -23).all()
    turn = np.angle(np.exp(1j * (np.arctan2(d64[1:, :, 1], d64[1:, :, 0]) - np.arctan2(d64[:-1, :, 1], d64[:-1, :, 0]) - 2 * np.pi / 16)))
    assert (np.abs(turn) * rad[1:] <= 2.0 ** -22).all()
    with pytest.raises(ValueError):
        I.ao_directions(17)


@pytest.mark.parametrize("spp", (1, 2, 4))
def test_rotation_index_covers_all_sixteen(I, spp):
    y, x = np.mgrid[0:9, 0:11]
    seen = np.zeros((9, 11, 16), bool)
    for frame_index in range(1, 16 // spp + 1):
        for k in range(spp):
            m = I.ao_rotation(x, y, frame_index, spp, k)
            assert m.min() >= 0 and m.max() <= 15 and not seen[y, x, m].any()
            seen[y, x, m] = True
    assert seen.all()
    # interleaved in one frame: a 4 x 4 block of pixels holds all sixteen
    assert sorted(I.ao_rotation(x[:4, :4], y[:4, :4], 3, spp, 0).ravel()) == list(range(16))


def test_basis_is_orthonormal_and_faces_the_viewer(I):
    rng = np.random.default_rng(5)
    n = rng.normal(size=(200, 3))
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F)
    n[:4] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]]
    T, B = I.ao_basis(n)
    for a, b, want in ((T, T, 1), (B, B, 1), (T, B, 0), (T, n, 0), (B, n, 0)):
        assert np.abs((a.astype(np.float64) * b).sum(1) - want).max() < 1e-6
    assert np.abs(np.cross(T.astype(np.float64), B) - n).max() < 1e-6
    d = rng.normal(size=(200, 3)).astype(F)
    N = I.ao_facing(n, d)
    assert ((N.astype(np.float64) * d).sum(1) <= 1e-7).all() and (np.abs(N) == np.abs(n)).all()
    assert np.isnan(I.ao_facing(np.full((1, 3), np.nan, F), d[:1])).all()
    # every ray of the table lies in the hemisphere of N
    D = I.ao_directions(16)
    for j in range(16):
        r = I.ao_ray(np.broadcast_to(D[3, j], (200, 3)), N, *I.ao_basis(N))
        assert ((r.astype(np.float64) * N).sum(1) > 0.17).all()


@pytest.mark.parametrize("K", (1, 5, 16))
@pytest.mark.parametrize("shading", (1, 2))
def test_a_plane_occludes_nothing(I, ovr, oracle, K, shading):
    """the neutral element: in front of a planar level set every walk finds nothing - O = 0 at every hit, the frame is the K = 0 frame bit for bit, colour and
    layer, although the AO walks walked"""
    vol = AC.ramp()
    off = _frame(I, ovr, oracle, vol, AC.RAMP_CAMERA, [0.5], shading=shading)
    on = _frame(I, ovr, oracle, vol, AC.RAMP_CAMERA, [0.5], ao=(I.ao_directions(K), INF), shading=shading)
    assert off[2]["hits"] > 100 and on[2]["ao_steps"] > 0 and on[2]["ao_fetched"] == on[2]["ao_steps"]
    assert np.array_equal(_bits(on[0]), _bits(off[0])) and np.array_equal(_bits(on[1]), _bits(off[1]))
    assert {k: v for k, v in on[2].items() if not k.startswith("ao_")} == {k: v for k, v in off[2].items() if not k.startswith("ao_")}
    basis = oracle.camera_basis(*AC.RAMP_CAMERA, AC.FOVY, *AC.SIZE).reshape(4, 3)
    d = ovr.projection.pixel_rays(basis, *AC.SIZE, None).reshape(-1, 3)
    r = I.trace_rays(vol, np.broadcast_to(basis[0], d.shape), d, 1.0, [0.5], ao=(I.ao_directions(K), INF, np.arange(len(d)) & 15))
    assert r["hit"].sum() > 100 and not r["flat"]["O"].any() and r["ao_steps"].sum() > r["hit"].sum()


@pytest.mark.parametrize("K", AC.KS)
def test_a_cavity_occludes_everything(I, ovr, oracle, K):
    """seen from inside a sphere every walk ends on the far wall: O = 1.0f exactly at EVERY hit (no grazing band is left out: the shortest chord, 2 r0 z_min,
    is 3.5 steps and the walks start 1.5 steps off the wall); with kd = ks = 0 the hits are black and opaque; cut at R = 2 the walks find nothing"""
    r = _cavity_events(I, K, INF)
    assert r["hit"].all() and np.array_equal(_bits(r["flat"]["O"]), _bits(np.ones(len(r["flat"]["O"]), F)))
    iso = [AC.level(AC.CAVITY_RADIUS)]
    vol = AC.cavity()
    on = _frame(I, ovr, oracle, vol, AC.CAVITY_CAMERA, iso, ao=(I.ao_directions(K), INF), material=(0.5, 0.0, 0.0, 0.0))
    assert (on[0][..., 3] == 1).all() and not on[0][..., :3].any()
    off = _frame(I, ovr, oracle, vol, AC.CAVITY_CAMERA, iso)
    short = _frame(I, ovr, oracle, vol, AC.CAVITY_CAMERA, iso, ao=(I.ao_directions(K), 2.0))
    assert short[2]["ao_steps"] > 0 and np.array_equal(_bits(short[0]), _bits(off[0])) and np.array_equal(_bits(short[1]), _bits(off[1]))
    lit = _frame(I, ovr, oracle, vol, AC.CAVITY_CAMERA, iso, ao=(I.ao_directions(K), INF))
    assert (lit[0][..., :3] <= off[0][..., :3]).all() and (lit[0][..., :3] < off[0][..., :3]).any()


def test_occlusion_grows_with_the_radius(I):
    """the walk to R1 is a prefix of the walk to R2 > R1: per event O(R1) <= O(R2)"""
    radii = (2.0, 6.0, 12.0, 19.0, 21.0, INF)
    O = [_cavity_events(I, 5, R, opacities=[0.4, 0.7], iso=[AC.level(AC.CAVITY_RADIUS), AC.level(AC.OUTER_RADIUS)])["flat"]["O"] for R in radii]
    assert all(len(o) == len(O[0]) for o in O) and not O[0].any()
    for a, b in zip(O, O[1:]):
        assert (a <= b).all()
    assert any((a < b).any() for a, b in zip(O, O[1:])) and len({o.tobytes() for o in O}) >= 3


@pytest.mark.parametrize("K", AC.KS)
@pytest.mark.parametrize("a", (0.25, 0.6))
def test_translucent_shells(I, K, a):
    """one shell of opacity a: every walk crosses it once, O is a to K ulp; two nested shells seen from inside both: 1 - (1 - a)^2"""
    one = _cavity_events(I, K, INF, opacities=[a])
    first = one["flat"]["O"][np.concatenate([[0], np.cumsum(one["n_events"])[:-1]])]
    assert one["hit"].all() and (_ulps(first, np.full(len(first), F(a))) <= K).all()
    two = _cavity_events(I, K, INF, opacities=[a, a], iso=[AC.level(AC.CAVITY_RADIUS), AC.level(AC.OUTER_RADIUS)])
    first = two["flat"]["O"][np.concatenate([[0], np.cumsum(two["n_events"])[:-1]])]
    want = F(fma32(F(1) - F(a), F(a), F(a)))
    assert (two["n_events"] == 2).all() and (_ulps(first, np.full(len(first), want)) <= K).all()
    assert abs(float(want) - (1 - (1 - a) ** 2)) < 1e-6


def fma32(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def test_range_skipping_is_invisible(I):
    """the skipping walk against the plain one, bit for bit, the counters' sums included - with isovalues at a macrocell's maximum and one ulp above it"""
    vol = AC.cavity()
    top = ovr_ranges_max(I, vol)
    for iso, opac in (([AC.level(AC.CAVITY_RADIUS)], None), ([AC.level(AC.CAVITY_RADIUS), AC.level(AC.OUTER_RADIUS)], [0.3, 0.8]), ([top], [0.5]),
                      ([np.nextafter(top, F(np.inf))], [0.5])):
        p = _cavity_events(I, 5, INF, opacities=opac, iso=iso)
        s = _cavity_events(I, 5, INF, opacities=opac, iso=iso, skipping=True)
        for key in ("hit", "steps", "n_events", "ao_steps", "shadow_steps"):
            assert np.array_equal(p[key], s[key]), (iso, key)
        for key in ("O", "t", "A", "shadow", "normal"):
            assert np.array_equal(_bits(p["flat"][key]), _bits(s["flat"][key])), (iso, key)
        assert (s["ao_fetched"] <= p["ao_fetched"]).all() and np.array_equal(p["ao_fetched"], p["ao_steps"])
    # every macrocell of the cavity holds its centre: there the rule drops steps only past the top.  A volume whose cells differ: steps are dropped, nothing moves
    vol = IC.volume("smooth", np.float32)
    org, d, _ = PC.ray_set(IC.DIMS[0])
    iso = IC.scaled(IC.ISOVALUES["smooth"], np.float32)
    ao = (I.ao_directions(5), 9.0, np.arange(len(org)) & 15)
    p = I.trace_rays(vol, org, d, 2.5, iso, opacities=[0.5, 0.3, 1.0], light=(0.3, 0.8, -0.52), ao=ao)
    s = I.trace_rays(vol, org, d, 2.5, iso, opacities=[0.5, 0.3, 1.0], light=(0.3, 0.8, -0.52), ao=ao, skipping=True)
    assert p["hit"].sum() > 10 and p["flat"]["O"].any() and np.array_equal(p["ao_steps"], s["ao_steps"]) and np.array_equal(_bits(p["flat"]["O"]), _bits(s["flat"]["O"]))
    assert s["ao_fetched"].sum() < p["ao_fetched"].sum() == p["ao_steps"].sum()


def ovr_ranges_max(I, vol):
    """the maximum of the macrocell at the cavity's centre"""
    from importlib import import_module
    P = import_module(I.__name__.rsplit(".", 1)[0] + ".projection")
    return F(P.macrocell_ranges(vol)[1, 1, 1, 1])


def test_the_setter_model_refuses_what_the_setter_refuses(I):
    for K in (-1, 17):
        with pytest.raises(ValueError):
            I.ao_directions(K)
    assert I.ao_directions(0).shape == (16, 0, 3)


def _quality(I, ovr, oracle, rate=1.0, size=(12, 10), R=INF, iso=0.2):
    """per hit of a small frame of the synthetic volume: the 16-rotation mean of O at K = 4, 8, 16, and the mean over a 4096-direction cosine-weighted sunflower
    (formed in float64 like the table) of the same walk"""
    n = 32
    vol = ovr.synth.make_volume(n, np.float32)
    eye, at, up = ovr.synth.make_camera("oblique", n)[:3]
    basis = oracle.camera_basis(eye, at, up, 45.0, *size).reshape(4, 3)
    d = ovr.projection.pixel_rays(basis, *size, None).reshape(-1, 3)
    org = np.broadcast_to(basis[0], d.shape)
    hit = I.trace_rays(vol, org, d, rate, [iso], shadows=False)["hit"]
    org, d = org[hit], d[hit]
    out = {}
    for K in (4, 8, 16):
        table = I.ao_directions(K)
        out[K] = np.mean([I.trace_rays(vol, org, d, rate, [iso], shadows=False, ao=(table, R, np.full(len(d), m)))["flat"]["O"].astype(np.float64) for m in range(16)], 0)
    j = np.arange(4096, dtype=np.float64)
    r2, phi = (j + 0.5) / 4096, 2 * np.pi * j * I.GOLDEN
    fine = np.stack([np.sqrt(r2) * np.cos(phi), np.sqrt(r2) * np.sin(phi), np.sqrt(1 - r2)], -1).astype(F)
    quad = np.zeros(len(d))
    for c in range(0, 4096, 16):        # sixteen directions per call (the model sums K <= 16 float32 terms: each chunk's mean is exact enough, the total is float64)
        chunk = np.broadcast_to(fine[c:c + 16], (16, 16, 3))
        quad += I.trace_rays(vol, org, d, rate, [iso], shadows=False, ao=(chunk, R, np.zeros(len(d), np.int64)))["flat"]["O"].astype(np.float64) / 256
    return out, quad


def test_occlusion_is_closer_to_the_quadrature_than_no_occlusion(I, ovr, oracle):
    """recorded, not tuned (the table is in DESIGN.md section 20): the mean |O - quadrature| is below the mean quadrature at K = 4, 8 and 16 - with ambient
    occlusion the ambient term is closer to the converged one than without"""
    got, quad = _quality(I, ovr, oracle)
    assert len(quad) >= 20 and quad.mean() > 0
    for K, O in got.items():
        print("K = %2d: mean O %.4f, mean quadrature %.4f, mean |O - quadrature| %.4f, max %.4f over %d hits" % (K, O.mean(), quad.mean(), np.abs(O - quad).mean(), np.abs(O - quad).max(), len(quad)))
        assert np.abs(O - quad).mean() < quad.mean(), K
