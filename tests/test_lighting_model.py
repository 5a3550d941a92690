"""The light and material model (open-volume-renderer_amd/lighting.py, include/ovr_hip.h ovr_hip_set_light / ovr_hip_set_material) on the CPU: the angle convention against the
reference's literal light, the reference material against the reference's literal expression, the guards that keep finite inputs finite, and the
four entry points in the header and in the library.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ["ovr_hip_set_light", "ovr_hip_set_material", "ovr_hip_get_lighting", "ovr_hip_shade_floats"]


@pytest.fixture(scope="module")
def lighting(ovr):
    return ovr.lighting


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.rad2deg(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1)))


def test_the_apps_default_angles_are_the_literal_light(lighting, oracle):
    lit = oracle.literals()
    literal = [lit["light_x"], lit["light_y"], lit["light_z"]]
    assert [float(x) for x in lighting.LITERAL_LIGHT] == literal  # the model's copy of the literal is the oracle's
    d = lighting.direction_from_angles(*lighting.APP_DEFAULT_ANGLES)
    assert d.dtype == np.float32
    assert _angle(d, literal) < 0.2
    # the two other readings of (phi, theta) are not the app's: y up, and phi measured from the equator
    p, t = np.deg2rad(lighting.APP_DEFAULT_ANGLES)
    assert _angle([np.sin(p) * np.cos(t), np.cos(p), np.sin(p) * np.sin(t)], literal) > 0.5
    assert _angle([np.cos(p) * np.cos(t), np.cos(p) * np.sin(t), np.sin(p)], literal) > 0.5


def test_angles_round_trip(lighting):
    phi, theta = lighting.angles_of(lighting.LITERAL_LIGHT)
    assert abs(phi - 99.521) < 1e-3 and abs(theta - 112.354) < 1e-3
    assert _angle(lighting.direction_from_angles(phi, theta), lighting.LITERAL_LIGHT) < 1e-4
    rng = np.random.default_rng(11)
    for phi, theta in zip(rng.uniform(1, 179, 200), rng.uniform(-179, 179, 200)):
        p2, t2 = lighting.angles_of(lighting.direction_from_angles(phi, theta))
        assert abs(p2 - phi) < 1e-4 and abs(t2 - theta) < 1e-4 / np.sin(np.deg2rad(phi))
    # a vector of any length has the angles of its direction
    assert np.allclose(lighting.angles_of([0, 0, 5]), (0, 0)) and np.allclose(lighting.angles_of([0, 3, 0]), (90, 90))


def test_normalize_is_the_host_routine(lighting, oracle):
    """float32 dot by two fused multiply-adds, sqrt, three divisions: the unit vector of the literal is what the oracle shades with - checked through
    the frame tests on the GPU; here: unit length to float precision, sign symmetry exact"""
    L = lighting.normalize(np.array(lighting.LITERAL_LIGHT, F))
    assert L.dtype == np.float32 and abs(float(np.linalg.norm(L.astype(np.float64))) - 1) < 2e-7
    assert np.array_equal(lighting.normalize(-np.array(lighting.LITERAL_LIGHT, F)), -L)


def test_fma_is_correctly_rounded(lighting):
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(3000) * 1e3).astype(F)
    b = rng.standard_normal(3000).astype(F)
    c = (-a * b * (1 + rng.standard_normal(3000).astype(F) * F(1e-6))).astype(F)  # heavy cancellation: where a double rounding would show
    got = lighting.fma(a, b, c)
    for i in range(3000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = F(float(exact))
        best = min((f, np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))), key=lambda v: abs(Fraction(float(v)) - exact))
        assert got[i] == best


def test_reference_material_is_the_literal_expression_bit_for_bit(lighting):
    rng = np.random.default_rng(7)
    n = 100000
    cos_nl, shadow = rng.random(n, dtype=F), rng.random(n, dtype=F)
    shadow[::7] = 0
    shadow[3::11] = 1
    want = lighting.reference_shade(cos_nl, shadow)
    # a normal along the light with |n| = cosNL gives exactly that cosine for the axis light
    L = np.array([0, 0, 1], F)
    normal = np.zeros((n, 3), F)
    normal[:, 2] = cos_nl * np.where(rng.random(n) < 0.5, F(-1), F(1))  # two-sided
    pos = rng.standard_normal((n, 3)).astype(F)
    for shininess in (0.0, 17.0):
        got = lighting.shade(normal, pos, shadow, L, (0, 0, 4), *lighting.REFERENCE_MATERIAL[:3], shininess, 1.0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # exact products: (ka .5, kd .25, intensity 2) and (.5, 1, .5)
    for kd, intensity in ((0.25, 2.0), (1.0, 0.5)):
        got = lighting.shade(normal, pos, shadow, L, (0, 0, 4), 0.5, kd, 0.0, 0.0, intensity)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and with the literal light: cosNL by the model's own dot
    Ll = lighting.normalize(np.array(lighting.LITERAL_LIGHT, F))
    nrm = lighting.normalize(rng.standard_normal((n, 3)).astype(F))
    c = np.abs(lighting.dot(np.broadcast_to(Ll, nrm.shape), nrm))
    assert np.array_equal(lighting.shade(nrm, pos, shadow, Ll, (0, 0, 4)).view(np.uint32), lighting.reference_shade(c, shadow).view(np.uint32))


def test_nan_normal_gives_nan_and_finite_inputs_stay_finite(lighting):
    L = lighting.normalize(np.array(lighting.LITERAL_LIGHT, F))
    cam = np.array([0.5, -2.0, 3.0], F)
    nan_n = np.full((4, 3), np.nan, F)
    pos = np.zeros((4, 3), F)
    for ks in (0.0, 0.4):
        assert np.isnan(lighting.shade(nan_n, pos, np.zeros(4, F), L, cam, 0.6, 0.9, ks, 40.0)).all()
    rng = np.random.default_rng(9)
    n = 4000
    nrm = lighting.normalize(rng.standard_normal((n, 3)).astype(F))
    pos = rng.standard_normal((n, 3)).astype(F)
    pos[:50] = cam                       # a sample at the camera: V = 0 / 0
    pos[50:100] = cam + L * F(2)         # V = -L: the half vector has length 0 (or nearly)
    H = lighting.normalize((L + lighting.normalize(cam - pos[100:200])).astype(F))
    t = np.cross(H, np.array([0.3, 0.5, 0.8], F)).astype(F)
    nrm[100:200] = lighting.normalize(t)  # perpendicular to H: cosNH = 0 or a rounding residue
    nrm[200:220] = nrm[200:220] * F(1e-39)  # denormal cosines
    shadow = rng.random(n, dtype=F)
    for shininess in (0.0, 1.0, 40.0, 100.0):
        s = lighting.shade(nrm, pos, shadow, L, cam, 0.6, 0.9, 0.4, shininess, 1.5)
        assert np.isfinite(s).all(), shininess
    assert np.array_equal(lighting.specular_power(np.array([0.0, 1e-39, np.nan], F), 0.0), np.zeros(3, F))   # the guard, not 0^0 or 0 * -inf
    assert lighting.specular_power(np.array([0.5], F), 0.0)[0] == 1.0 and lighting.specular_power(np.array([1.0], F), 40.0)[0] == 1.0
    assert abs(float(lighting.specular_power(np.array([0.5], F), 3.0)[0]) - 0.125) < 1e-7


def test_shade_is_monotone_in_ks(lighting):
    rng = np.random.default_rng(13)
    n = 5000
    L = lighting.normalize(np.array([1, -1, 0.2], F))
    nrm = lighting.normalize(rng.standard_normal((n, 3)).astype(F))
    pos, shadow = rng.standard_normal((n, 3)).astype(F), rng.random(n, dtype=F)
    prev = lighting.shade(nrm, pos, shadow, L, (0, 0, 3), 0.3, 0.7, 0.0, 20.0)
    for ks in (1e-3, 0.1, 0.4, 1.0, 5.0):
        cur = lighting.shade(nrm, pos, shadow, L, (0, 0, 3), 0.3, 0.7, ks, 20.0)
        assert (cur >= prev).all()
        prev = cur
    assert (prev > lighting.shade(nrm, pos, shadow, L, (0, 0, 3), 0.3, 0.7, 0.0, 20.0)).any()


def test_header_declares_and_library_exports_the_entry_points(ovr):
    hdr = open(os.path.join(ROOT, "include", "ovr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ovr._lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in ovr._lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct ovr_hip_lighting" in code
    import ctypes as C
    assert C.sizeof(ovr._lib.Lighting) == 9 * 4
    # (added within the ABI version that was current: nothing that existed changed, tests/test_abi.py compares the version with the library's)
    assert int(re.search(r"#define OVR_HIP_ABI_VERSION (\d+)", hdr).group(1)) == ovr._lib.EXPECTED_ABI == lib.ovr_hip_abi_version()
    # argument checks need no device
    assert lib.ovr_hip_set_light(None, None, 1.0) < 0 and lib.ovr_hip_set_material(None, 0.5, 0.5, 0.0, 0.0) < 0
    assert lib.ovr_hip_get_lighting(None, None) < 0 and lib.ovr_hip_shade_floats(None, None, None, None, None, 0) < 0
