"""Pins the oracle's MARCHING arithmetic to the reference's own shader text.

tests/golden/ref_march.npz (tests/golden/make_ref_march.py) holds what the reference's shaders_raymarching.cu + shaders_common.h compute
when compiled, unmodified, for the host (oracle/ref_march_probe.cpp over oracle/cuda_host_shim/): frames and iteration counts of two
builds, without and with contraction of a * b + c.  The reference does not fix where nvcc contracts; the two builds bracket that freedom.

The bar, fixed before anything was compared: per quantity (alpha, premultiplied colour, premultiplied gradient) D = the largest difference
between the two builds over ALL scenes of the fixture; the oracle - a third contraction pattern - must stay within 4 x D of the NEARER
build, element by element, and its primary and shadow iteration counts must EQUAL the reference's.  Measured values: ref_march_notes.md."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ref_march_scenes as RS
from ref_march_common import noise_tile_for
from test_oracle_spec import Spec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES, D = RS.load_fixture(os.path.join(HERE, "golden", "ref_march.npz"))
IDS = [s["name"] for s in SCENES]


def oracle_render(O, s, **override):
    """the oracle on a fixture scene (default pow mode, every sample shaded) -> rgba, grad, primary iterations, shadow iterations over all frames"""
    import ctypes as C
    p = dict(s)
    p.update(override)
    w, h = p["size"]
    sparse = len(p["pixels"]) > 0
    sc = O.OracleScene(p["vol"], p["colors"], p["alphas"], p["vr"], p["cam"], w, h, fovy=p["fovy"], spp=p["spp"], rate=p["rate"], shading=O.SHADE_FULL,
                       grid_origin=p["origin"], grid_spacing=p["spacing"], convention=O.GRID_CELL, sparse=sparse, noise=noise_tile_for(p) if sparse else None,
                       skip_zero_opacity=False)
    rgba, grad, accum = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.float32)
    primary = shadow = 0
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for f in range(1, p["frames"] + 1):
        if sparse and not p["accumulate"]:
            rgba[:], grad[:] = 0, 0
        cnt = O.Counters()
        sc.lib.ovr_oracle_render_frame(C.byref(sc.s), f, int(bool(p["accumulate"])), fp(accum), fp(rgba), fp(grad), C.byref(cnt), 0)
        primary += cnt.samples
        shadow += cnt.shadow_samples
    return rgba, grad, primary, shadow


def failures(s, rgba, grad, primary, shadow):
    """every way in which a rendering of scene `s` misses the bar; empty = it passes"""
    out = []
    if primary != s["primary"]:
        out.append(f"primary iterations {primary} != {s['primary']}")
    if shadow != s["shadow"]:
        out.append(f"shadow iterations {shadow} != {s['shadow']}")
    ref_nan = np.isnan(s["rgba"]).any() or np.isnan(s["grad"]).any()
    if not ref_nan and (np.isnan(rgba).any() or np.isnan(grad).any()):
        out.append("NaN where the reference has none")
    pixels = s["pixels"] if len(s["pixels"]) else None
    for q, (dist, tol, ratio) in RS.band_excess(s, D, rgba, grad, pixels=pixels).items():
        if ratio > 1.0:
            out.append(f"{q}: {dist:.3e} from the nearer build, band {tol:.3e}")
    if pixels is not None:   # nothing outside the list may be written
        mask = np.ones(rgba.shape[:2], bool)
        mask[pixels[:, 1], pixels[:, 0]] = False
        if np.any(rgba[mask] != 0) or np.any(s["rgba"][mask] != 0):
            out.append("a pixel outside the sparse list was written")
    return out


def test_the_scene_list_reaches_what_it_must():
    by = lambda f: [s for s in SCENES if f(s)]
    assert {s["dtype"] for s in SCENES} == set(RS.DTYPES)
    assert {0.5, 1.0, 4.0, 20.0} <= {s["rate"] for s in SCENES}
    assert by(lambda s: tuple(s["spacing"]) != (1.0, 1.0, 1.0) and tuple(s["origin"]) != (0.0, 0.0, 0.0))
    assert by(lambda s: s["cam_kind"] == "inside") and by(lambda s: s["cam_kind"] in ("front", "above", "top") and s["size"][0] % 2 == 1 and s["size"][1] % 2 == 1)
    assert by(lambda s: s["const_region"]) and by(lambda s: s["spp"] == 3) and by(lambda s: s["frames"] == 3 and s["accumulate"]) and by(lambda s: len(s["pixels"]) > 0)
    assert {(2, 2), (16, 16), (1024, 1024)} <= {tuple(s["tables"][:2]) for s in SCENES} and by(lambda s: s["tables"][0] != s["tables"][1])
    assert max(max(s["dims"]) for s in SCENES) == 24 and 38 <= len(SCENES) <= 48
    for s in SCENES:   # every scene shows something, and D is a property of the whole fixture
        assert s["primary"] > 0 and s["shadow"] > 0 and float(s["rgba"][..., 3].max()) > 0.05, s["name"]
    assert all(D[q] > 0 for q in RS.QUANTITIES), D


@pytest.mark.parametrize("s", SCENES, ids=IDS)
def test_oracle_matches_the_reference_shader(oracle, s):
    assert oracle.load().ovr_oracle_get_powf_mode() == oracle.POWF_EXP2_LOG2
    rgba, grad, primary, shadow = oracle_render(oracle, s)
    ex = RS.band_excess(s, D, rgba, grad, pixels=s["pixels"] if len(s["pixels"]) else None)
    print(f"{s['name']}: " + ", ".join(f"{q} {d:.2e} / {t:.2e}" for q, (d, t, _) in ex.items()))
    bad = failures(s, rgba, grad, primary, shadow)
    assert not bad, f"{s['name']}: " + "; ".join(bad)


SPEC_SCENES = [s for s in SCENES if s["dtype"] in ("f32", "u8") and s["spp"] == 1 and s["frames"] == 1 and not len(s["pixels"]) and s["vr"][1] >= s["vr"][0]]


@pytest.mark.parametrize("s", SPEC_SCENES, ids=[s["name"] for s in SPEC_SCENES])
def test_float64_spec_matches_the_reference_shader(s):
    """the independent float64 implementation of test_oracle_spec.py on the scenes it can express (float32 / uint8, one sample per pixel, one dense
    frame, a valid value range): the same 4 x D band, with the 5e-5 it is held to against the oracle as an upper limit.

    Counts: float64 cannot reproduce a float32 tie at the exit of the box - whether a last sliver of a step, narrower than the rounding of t, exists.
    That is at most one iteration per ray, so the total may differ by at most the number of rays; it is printed.  (The oracle's counts must be EQUAL.)

    The spec marches from the camera the shader is handed: the twelve floats the reference's host math stores in the launch parameters, kept in the fixture
    (they are the shader's input, like the voxels; the host formulas are pinned on their own in tests/test_oracle_vs_ref.py).  Deriving the basis from the
    application's camera in float64 instead moves the rays by the stored floats' last bits, which a steep table turns into up to 5.4e-5 of alpha (f32_subrange:
    one float step of the eye is 4.4e-6 there) - a difference of inputs, not of marching arithmetic.  Measured with the stored basis: worst scene f32_subrange,
    alpha 4.32e-5 (band 5e-5), premultiplied colour 3.10e-5 (band 3.37e-5); next tables_1024_1024 with 2.41e-5 / 1.30e-5."""
    sp = Spec(s["vol"], s["colors"], s["alphas"], s["vr"], s["cam"], s["size"], s["fovy"], s["rate"], 2, origin=s["origin"], spacing=s["spacing"], basis=s["basis"])
    w, h = s["size"]
    rgba = np.zeros((h, w, 4), np.float32)
    n_tot = 0
    for iy in range(h):
        for ix in range(w):
            px, n, _ = sp.ray(ix, iy)
            rgba[iy, ix] = px
            n_tot += n
    ex = RS.band_excess(s, D, rgba, np.zeros((h, w, 3), np.float32), cap=5e-5, which=("alpha", "colour"))
    print(f"{s['name']}: spec iterations {n_tot} vs {s['primary']}; " + ", ".join(f"{q} {d:.2e} / {t:.2e}" for q, (d, t, _) in ex.items()))
    assert abs(n_tot - s["primary"]) <= w * h, (n_tot, s["primary"])
    assert all(r <= 1.0 for _, _, r in ex.values()), (s["name"], ex)


def test_a_fresh_run_of_the_probes_reproduces_the_fixture():
    """so that the fixture cannot drift from its recipe; needs the binaries oracle/build_ref.sh makes where the reference tree is present"""
    import make_ref_march as G
    if not G.probes_present():
        pytest.skip("oracle/_ref/ref_march_probe* not built (no reference tree here)")
    fresh, _ = G.generate()
    z = np.load(os.path.join(HERE, "golden", "ref_march.npz"))
    assert sorted(fresh) == sorted(z.files)
    for k in z.files:
        assert fresh[k].dtype == z[k].dtype and np.array_equal(fresh[k], z[k]), k
    with tempfile.TemporaryDirectory() as d:
        G.save_deterministic(os.path.join(d, "a.npz"), fresh)
        with open(os.path.join(d, "a.npz"), "rb") as a, open(os.path.join(HERE, "golden", "ref_march.npz"), "rb") as b:
            assert a.read() == b.read(), "the file itself is not reproduced byte for byte"


def _first(name):
    return next(s for s in SCENES if s["name"] == name)


@pytest.mark.parametrize("what", ["light_x_sign", "light_z_sign", "rate_1.01", "colour_table_shifted", "alpha_table_shifted"])
def test_the_pin_bites(oracle, what):
    """perturb the oracle's input the way a misreading of the shader would: the comparison that passes above must FAIL"""
    s = _first("f32_subrange") if what == "alpha_table_shifted" else _first("f32_oblique")
    assert s["rate"] == 1.0
    assert not failures(s, *oracle_render(oracle, s))
    lit = oracle.literals()
    light = [lit["light_x"], lit["light_y"], lit["light_z"]]
    import ctypes as C
    set_light = oracle.load().ovr_oracle_set_light_for_selfcheck
    set_light.argtypes = [C.POINTER(C.c_float)]
    try:
        if what.startswith("light"):
            k = "xyz".index(what[6])
            light[k] = -light[k]
            set_light((C.c_float * 3)(*light))
            got = oracle_render(oracle, s)
        elif what == "rate_1.01":
            got = oracle_render(oracle, s, rate=1.01)
        elif what == "colour_table_shifted":
            got = oracle_render(oracle, s, colors=np.roll(s["colors"].reshape(-1, 3), 1, axis=0).ravel())
        else:
            a = s["alphas"].reshape(-1, 2).copy()
            a[:, 1] = np.roll(a[:, 1], 1)
            got = oracle_render(oracle, s, alphas=a.ravel())
    finally:
        set_light(None)
    bad = failures(s, *got)
    assert bad, f"{what}: the comparison did not notice"
    if what.startswith("light") or what == "colour_table_shifted":   # no primary count and no opacity changes: the COLOUR band has to catch these
        assert any(b.startswith("colour") for b in bad) and not any(b.startswith("primary") or b.startswith("alpha") for b in bad), bad
