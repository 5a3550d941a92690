"""Light and material on the GPU (include/ovr_hip.h ovr_hip_set_light / ovr_hip_set_material): the defaults change nothing, every light direction agrees with the
CPU oracle (given the same raw vector through its self-check hook), the frame does not depend on pipeline / layout / addressing / skipping / shade order /
device group under a non-default light and a specular material, the material is linear where the model says so, ovr_hip_shade_floats reproduces
lighting.py, and the setters behave like every other setter.  Under the exact-parity build the oracle comparisons and the shade function are EQUALITY."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import EXACT_RUN, compare, hip_frame, hip_setup, make_case, oracle_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
RENDERBATCH = os.path.join(ROOT, "oracle", "_ref", "renderbatch")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
F = np.float32

# ovr_hip_shade_floats of the PRODUCT against lighting.py: the largest absolute difference measured on the MI355X over the triples of
# test_shade_function_vs_model (profiles/r08_lighting.md section 2) - v_rsq_f32 twice, v_log_f32, v_exp_f32 in the specular term.  The bar is four times it.
# (The figure is the one of shininess 40, the largest the one run that reached a GPU reported; shininess 100 had not been measured then.)
MEASURED_SHADE_DIFF = 1.621e-5
SHADE_BAR = 4 * MEASURED_SHADE_DIFF

SPECULAR = (0.6, 0.9, 0.4, 40.0)  # the interactive app's default material
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")


def _counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


def _literal(oracle):
    lit = oracle.literals()
    return [lit["light_x"], lit["light_y"], lit["light_z"]]


def _lights(ovr, oracle):
    lit = _literal(oracle)
    return {"+z": [0, 0, 1], "-x": [-1, 0, 0], "-y": [0, -1, 0], "111": [1, 1, 1], "1-10": [1, -1, 0],
            "app": [float(x) for x in ovr.lighting.direction_from_angles(*ovr.lighting.APP_DEFAULT_ANGLES)], "-literal": [-x for x in lit]}


class oracle_light:
    """the oracle's light for the duration of a block; the hook is process-wide, so the literal comes back whatever happens"""

    def __init__(self, oracle, vec):
        self.fn = oracle.load().ovr_oracle_set_light_for_selfcheck
        self.fn.argtypes = [C.POINTER(C.c_float)]
        self.fn.restype = None
        self.vec = vec

    def __enter__(self):
        self.fn((C.c_float * 3)(*[float(x) for x in self.vec]))

    def __exit__(self, *a):
        self.fn(None)


SCENES = {
    "sparse_front_f32": dict(n=32, tf="sparse", cam="front", dtype=np.float32),
    "dense_oblique_u8": dict(n=32, tf="dense", cam="oblique", dtype=np.uint8),
    "sparse_oblique_u16_aniso": dict(n=0, dims=(40, 23, 31), tf="sparse", cam="oblique", dtype=np.uint16, spacing=(1.0, 1.5, 0.75), origin=(3.0, -2.0, 5.0)),
    "dense_front_f32": dict(n=32, tf="dense", cam="front", dtype=np.float32),
}


# ---- 1. the defaults are untouched -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("pipeline", [1, 2])
def test_defaults_untouched(ovr, oracle, hip_renderer_factory, pipeline, skip):
    case = make_case(ovr, oracle, n=40, tf="bumps", cam="oblique", size=(96, 64), shading=2)
    lit = _literal(oracle)
    variants = {
        "nothing called": lambda r: None,
        "NULL light + reference material": lambda r: (r.set_light_direction(None, 1.0), r.set_material(0.5, 0.5, 0.0, 33.0)),
        "the literal as a vector": lambda r: r.set_light_direction(lit, 1.0),
        "ka .5 kd .25 intensity 2": lambda r: (r.set_material(0.5, 0.25, 0.0, 0.0), r.set_light_direction(None, 2.0)),
        "ka .5 kd 1 intensity .5": lambda r: (r.set_material(0.5, 1.0, 0.0, 0.0), r.set_light_direction(None, 0.5)),
    }
    got = {}
    for name, setup in variants.items():
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        ren.set_empty_space_skipping(skip)
        setup(ren)
        ren.commit()
        ren.render()
        got[name] = hip_frame(ovr, ren) + (_counters(ren.stats()), ren.lighting().is_reference)
        ren.close()
    base = got["nothing called"]
    for name, (rgba, grad, cnt, is_ref) in got.items():
        assert np.array_equal(rgba.view(np.uint32), base[0].view(np.uint32)), name
        assert np.array_equal(grad.view(np.uint32), base[1].view(np.uint32)), name
        assert cnt == base[2], (name, cnt, base[2])
    assert [got[k][3] for k in list(variants)[:3]] == [1, 1, 1] and got["ka .5 kd .25 intensity 2"][3] == 0
    assert base[0][..., :3].max() > 0.1
    ref, _, cnt = oracle_scene(oracle, case).render()
    compare(oracle, base[0], ref, name="defaults")
    assert base[2][1] + base[2][5] == cnt.samples


# ---- 2. every light direction against the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("light", ["+z", "-x", "-y", "111", "1-10", "app", "-literal"])
def test_light_direction_vs_oracle(ovr, oracle, hip_renderer_factory, light, scene):
    case = make_case(ovr, oracle, size=(64, 48), shading=2, **SCENES[scene])
    vec = _lights(ovr, oracle)[light]
    with oracle_light(oracle, vec):
        ref, ref_grad, cnt = oracle_scene(oracle, case).render()
    ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=2 if light in ("+z", "111", "app") else 1)
    ren.set_light_direction(vec)
    ren.commit()
    ren.render()
    rgba, grad = hip_frame(ovr, ren)
    st = ren.stats()
    ren.close()
    print(f"{scene} / {light}: max float difference {np.abs(rgba - ref).max():.3g}, shadow samples {st.shadow_samples} (oracle {cnt.shadow_samples_visible}), shaded {st.shaded_samples}")
    assert np.isfinite(ref).all() and cnt.shadow_samples_visible > 0
    compare(oracle, rgba, ref, name=f"{scene}/{light}")
    assert st.rays == cnt.rays
    assert st.samples == cnt.samples, "primary sample count differs from the oracle"
    assert st.shaded_samples == cnt.shaded_samples
    if EXACT_RUN:  # the product: no bar on the shadow count (tests/test_config_sweep_gpu.py); the same arithmetic on both sides: equal
        assert st.shadow_samples == cnt.shadow_samples_visible
        assert np.array_equal(grad.view(np.uint32), ref_grad.view(np.uint32))


# ---- 3. invariants under a non-default light and a specular material ---------------------------------------------------------------------------

def _lit_frame(ovr, ren, case, light=(1.0, -1.0, 0.3), material=SPECULAR, intensity=1.3, **setup):
    hip_setup(ovr, ren, case, **setup)
    ren.set_light_direction(light, intensity)
    ren.set_material(*material)
    return ren


def test_invariant_pipelines_skipping_layouts(ovr, oracle, hip_renderer_factory):
    case = make_case(ovr, oracle, n=40, tf="bumps", cam="oblique", size=(96, 64), shading=2)
    frames = {}
    for pipeline in (1, 2):
        for skip in (False, True):
            for layout in (0, 1, 2, 3):
                if layout and (pipeline, skip) not in ((1, False), (2, True)):
                    continue
                ren = hip_renderer_factory()
                ren.set_volume_layouts(2)
                ren.set_layout_choice(layout)
                _lit_frame(ovr, ren, case, pipeline=pipeline)
                ren.set_empty_space_skipping(skip)
                ren.commit()
                ren.render()
                st = ren.stats()
                assert st.layout == layout and st.pipeline == pipeline
                frames[(pipeline, skip, layout)] = hip_frame(ovr, ren) + ((st.rays, st.samples + st.skipped_samples, st.shaded_samples, st.shadow_samples + st.skipped_shadow_samples),)
                ren.close()
    base = frames[(1, False, 0)]
    for k, (rgba, grad, cnt) in frames.items():
        assert np.array_equal(rgba.view(np.uint32), base[0].view(np.uint32)), k
        assert np.array_equal(grad.view(np.uint32), base[1].view(np.uint32)), k
        assert cnt == base[2], k
    # ... and it is not the reference state's frame
    ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=1)
    ren.render()
    assert np.abs(hip_frame(ovr, ren)[0] - base[0]).max() > 0.05
    ren.close()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_invariant_addressing_modes(ovr, oracle, hip_renderer_factory, monkeypatch, dtype):
    case = make_case(ovr, oracle, n=40, tf="bumps", cam="oblique", size=(72, 56), shading=2, dtype=dtype)
    frames = []
    for am in (0, 1, 2, 3):
        monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
        for pipeline in (2, 1):
            ren = _lit_frame(ovr, hip_renderer_factory(), case, pipeline=pipeline)
            ren.commit()
            ren.render()
            frames.append(hip_frame(ovr, ren)[0].copy())
            ren.close()
    for f in frames[1:]:
        assert np.array_equal(f.view(np.uint32), frames[0].view(np.uint32))


def test_invariant_shade_order(ovr, oracle, hip_renderer_factory, monkeypatch):
    case = make_case(ovr, oracle, n=48, tf="dense", cam="oblique", size=(128, 96), shading=2)
    frames = []
    for order in ("0", None):
        if order is None:
            monkeypatch.delenv("OVR_HIP_SHADE_ORDER", raising=False)
        else:
            monkeypatch.setenv("OVR_HIP_SHADE_ORDER", order)   # read when the renderer is created
        for light in ((1.0, -1.0, 0.3), (0.0, 0.0, 1.0)):       # an axis light: the beam grid's degenerate-looking case
            ren = _lit_frame(ovr, hip_renderer_factory(), case, light=light, pipeline=2)
            ren.commit()
            ren.render()
            assert ren.stats().pipeline == 2
            frames.append(hip_frame(ovr, ren)[0].copy())
            ren.close()
    assert np.array_equal(frames[0].view(np.uint32), frames[2].view(np.uint32)) and np.array_equal(frames[1].view(np.uint32), frames[3].view(np.uint32))
    assert not np.array_equal(frames[0], frames[1])


def test_invariant_device_group(ovr, oracle, hip_renderer_factory):
    case = make_case(ovr, oracle, n=40, tf="bumps", cam="oblique", size=(97, 61), shading=2)

    def run(ren):
        _lit_frame(ovr, ren, case, accumulate=True)
        ren.commit()
        for _ in range(2):
            ren.render()
        a = hip_frame(ovr, ren) + (_counters(ren.stats()),)
        ren.set_light_direction((0.2, 1.0, -0.4), 0.8)   # forwarded to every member, resets every member's accumulation
        ren.commit()
        ren.render()
        assert ren.stats().frame_index == 1
        return a, hip_frame(ovr, ren) + (_counters(ren.stats()),), ren.lighting()

    single = hip_renderer_factory()
    want = run(single)
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        got = run(group)
    finally:
        group.close()
    for k in range(2):
        assert np.array_equal(got[k][0].view(np.uint32), want[k][0].view(np.uint32)), k
        assert np.array_equal(got[k][1].view(np.uint32), want[k][1].view(np.uint32)), k
        assert got[k][2] == want[k][2], k
    assert list(got[2].direction) == list(want[2].direction) and got[2].intensity == want[2].intensity
    assert not np.array_equal(want[0][0], want[1][0])
    single.close()


# ---- 4. the material against the oracle ----------------------------------------------------------------------------------------------------------

def _half_colour_case(ovr, oracle, shading=2, **kw):
    case = make_case(ovr, oracle, n=32, size=(64, 48), shading=shading, **kw)
    case["colors"] = (np.asarray(case["colors"], F) * F(0.5)).astype(F)   # the synthetic tables reach 1.0: clamp01 would break linearity
    return case


def _render(ovr, ren, case, material, intensity=1.0, light=None, **setup):
    hip_setup(ovr, ren, case, **setup)
    ren.set_material(*material)
    ren.set_light_direction(light, intensity)
    ren.commit()
    ren.render()
    out = hip_frame(ovr, ren) + (_counters(ren.stats()),)
    ren.close()
    return out


@pytest.mark.parametrize("tf,cam", [("dense", "oblique"), ("sparse", "front")])
def test_half_material_is_half_the_frame_vs_oracle(ovr, oracle, hip_renderer_factory, tf, cam):
    case = _half_colour_case(ovr, oracle, tf=tf, cam=cam)
    ref, ref_grad, cnt = oracle_scene(oracle, case).render()
    rgba, grad, counters = _render(ovr, hip_renderer_factory(), case, (0.25, 0.25, 0.0, 0.0), pipeline=2)
    doubled = rgba.copy()
    doubled[..., :3] *= F(2)   # exact
    assert ref[..., :3].max() > 0.05
    compare(oracle, doubled, ref, name=f"half material {tf}/{cam}")
    assert counters[1] == cnt.samples and counters[2] == cnt.shaded_samples


def test_ambient_and_diffuse_frames_add_up(ovr, oracle, hip_renderer_factory):
    case = _half_colour_case(ovr, oracle, tf="dense", cam="oblique")
    ref, _, _ = oracle_scene(oracle, case).render()
    amb = _render(ovr, hip_renderer_factory(), case, (0.5, 0.0, 0.0, 0.0), pipeline=1)
    dif = _render(ovr, hip_renderer_factory(), case, (0.0, 0.5, 0.0, 0.0), pipeline=1)
    both = amb[0].copy()
    both[..., :3] += dif[0][..., :3]
    a8, b8 = oracle.rgba8(both), oracle.rgba8(ref)
    df = np.abs(both - ref).max()
    print(f"ambient + diffuse against the oracle: max float difference {df:.3g}")
    # helpers.compare's bar, spelled out: under the exact-parity run that function demands equality, which a sum of two frames cannot give
    assert np.abs(a8.astype(int) - b8.astype(int)).max() <= 1 and df <= 2e-4 and not np.isnan(both).any()
    assert dif[0][..., :3].max() > 0.02 and np.array_equal(amb[0][..., 3], dif[0][..., 3])


def test_specular_only_adds_light_and_material_leaves_the_rest_alone(ovr, oracle, hip_renderer_factory):
    case = _half_colour_case(ovr, oracle, tf="dense", cam="oblique")
    base = _render(ovr, hip_renderer_factory(), case, (0.5, 0.5, 0.0, 0.0), pipeline=2)
    prev = base
    for ks, sh in ((0.05, 40.0), (0.4, 40.0), (0.4, 1.0), (0.4, 0.0)):
        cur = _render(ovr, hip_renderer_factory(), case, (0.5, 0.5, ks, sh), pipeline=2)
        assert (cur[0][..., :3] >= base[0][..., :3]).all(), (ks, sh)      # rounding is monotone: exactly
        assert np.array_equal(cur[0][..., 3].view(np.uint32), base[0][..., 3].view(np.uint32))   # alpha,
        assert np.array_equal(cur[1].view(np.uint32), base[1].view(np.uint32))                    # the gradient layer
        assert cur[2] == base[2]                                                                    # and every counter do not know the material
        prev = cur
    assert (prev[0][..., :3] > base[0][..., :3]).any()
    for m in ((0.1, 2.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)):
        cur = _render(ovr, hip_renderer_factory(), case, m, intensity=3.0, pipeline=1)
        assert np.array_equal(cur[0][..., 3], base[0][..., 3]) and np.array_equal(cur[1], base[1]) and cur[2] == base[2]
    assert cur[0][..., :3].max() == 0.0   # no ambient, no diffuse, no specular: black, with the same alpha


def test_gradient_shading_specular_with_shininess_0_is_ambient(ovr, oracle, hip_renderer_factory):
    """under SHADE_GRADIENT shadow = 0 and x^0 = 1: (0, 0, ks, 0) is the constant ks * I2 - the frame of (ka = ks * I2, 0, 0) bit for bit (pixels whose
    normal is NaN are 0 in both: NaN reaches shade through cosNL = NaN * 0 ... and through sp's guard respectively - see the assertion on them)"""
    case = _half_colour_case(ovr, oracle, shading=1, tf="dense", cam="oblique")
    ks, intensity = 0.375, 0.5
    spec = _render(ovr, hip_renderer_factory(), case, (0.0, 0.0, ks, 0.0), intensity=intensity, pipeline=2)
    amb = _render(ovr, hip_renderer_factory(), case, (ks * 2 * intensity, 0.0, 0.0, 0.0), intensity=intensity, pipeline=2)
    assert np.array_equal(spec[0].view(np.uint32), amb[0].view(np.uint32))
    assert spec[0][..., :3].max() > 0.02 and spec[2] == amb[2]


# ---- 5. the shade function itself ------------------------------------------------------------------------------------------------------------------

def _triples(ovr, L, cam, seed=17, n=6000):
    lighting = ovr.lighting
    rng = np.random.default_rng(seed)
    nrm = lighting.normalize(rng.standard_normal((n, 3)).astype(F))
    pos = (rng.standard_normal((n, 3)) * 20).astype(F)
    shadow = rng.random(n, dtype=F)
    shadow[::5] = 0
    H = lighting.normalize((L + lighting.normalize((cam - pos[:300]).astype(F))).astype(F))
    nrm[:300] = lighting.normalize(np.cross(H, np.array([0.3, 0.5, 0.8], F)).astype(F))   # perpendicular to H
    nrm[300:340] = np.nan                                                                   # zero gradients
    nrm[340:350, 0] = np.nan
    pos[350:400] = cam                                                                      # at the camera
    pos[400:430] = (cam + L * F(7)).astype(F)                                               # V = -L
    nrm[430:460] = nrm[430:460] * F(1e-39)                                                  # denormal cosines
    nrm[460:520] = H[:60]                                                                   # the highlight's peak
    return nrm, pos, shadow


@pytest.mark.parametrize("shininess", [0.0, 1.0, 40.0, 100.0])
def test_shade_function_vs_model(ovr, oracle, hip_renderer_factory, shininess):
    lighting = ovr.lighting
    case = make_case(ovr, oracle, n=16, tf="dense", cam="oblique", size=(32, 24), shading=2)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    raw = (1.0, -2.0, 0.5)
    cam = np.array(case["cam"][0], F)
    worst = 0.0
    for material, intensity in (((0.6, 0.9, 0.4, shininess), 1.5), ((0.5, 0.5, 0.0, shininess), 1.0), ((0.0, 0.0, 2.0, shininess), 1.0)):
        ren.set_material(*material)
        ren.set_light_direction(raw, intensity)
        ren.commit()
        L = np.array(list(ren.lighting().direction), F)
        assert np.array_equal(L, lighting.normalize(np.array(raw, F)))    # the unit vector the kernels use is the model's
        nrm, pos, shadow = _triples(ovr, L, cam)
        got = ren.shade_floats(nrm, pos, shadow)
        want = lighting.shade(nrm, pos, shadow, L, cam, *material, intensity)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(want).sum() == 50 and np.isfinite(want[~np.isnan(want)]).all()
        ok = ~np.isnan(want)
        if material[2] == 0.0 and ovr._lib.load().ovr_hip_built_for_exact_parity() == 0:
            # no specular term: the product's arithmetic is the model's too
            assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
        d = float(np.abs(got[ok] - want[ok]).max())
        rel = float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-30)).max())
        print(f"shade_floats vs lighting.py, shininess {shininess}, material {material}, intensity {intensity}: max abs difference {d:.4g}, max relative {rel:.4g}")
        worst = max(worst, d)
        if ovr._lib.load().ovr_hip_built_for_exact_parity() == 1:
            assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), f"{int((got[ok].view(np.uint32) != want[ok].view(np.uint32)).sum())} of {int(ok.sum())} differ"
    if ovr._lib.load().ovr_hip_built_for_exact_parity() == 0:
        assert worst <= SHADE_BAR, (worst, SHADE_BAR)
    ren.close()


# ---- 6. the state machine --------------------------------------------------------------------------------------------------------------------------

def test_setters_reset_accumulation_and_estimate(ovr, oracle, hip_renderer_factory):
    case = make_case(ovr, oracle, n=32, tf="dense", cam="oblique", size=(64, 48), shading=2, spp=2)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    ren.set_convergence(1, 0.0)
    ren.commit()
    for action in (lambda: ren.set_light_direction((0, 0, 1)), lambda: ren.set_material(*SPECULAR), lambda: ren.set_light_phi(60.0), lambda: ren.set_mat_shininess(8.0),
                   lambda: ren.set_light_intensity(2.0)):
        while ren.stats().frame_index < 4:
            ren.render()
        assert ren.stats().frame_index == 4 and ren.convergence().valid == 1
        before = hip_frame(ovr, ren)[0]
        action()
        ren.render()                      # queued: nothing happens before the commit
        assert ren.stats().frame_index == 5
        ren.commit()
        assert ren.convergence().valid == 0
        ren.render()
        assert ren.stats().frame_index == 1
        assert not np.array_equal(hip_frame(ovr, ren)[0], before)
    # the same values again: nothing changed, nothing is reset
    ren.render()
    ren.set_material(*ren._material)
    ren.set_light_intensity(2.0)
    ren.commit()
    ren.render()
    assert ren.stats().frame_index == 3
    ren.close()


def test_einval_leaves_the_state_unchanged_and_get_lighting_reports_the_frame(ovr, oracle, hip_renderer_factory):
    lighting = ovr.lighting
    case = make_case(ovr, oracle, n=24, tf="dense", cam="oblique", size=(48, 32), shading=2)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    s0 = ren.lighting()
    assert s0.is_reference == 1 and (s0.ambient, s0.diffuse, s0.specular, s0.intensity) == (0.5, 0.5, 0.0, 1.0)
    assert np.array_equal(np.array(list(s0.direction), F), lighting.normalize(np.array(lighting.LITERAL_LIGHT, F)))
    ren.set_light_direction((3.0, 0.0, 4.0), 1.25)
    ren.set_material(0.25, 0.75, 0.5, 12.0)
    assert ren.lighting().is_reference == 1          # queued, not committed
    ren.commit()
    ren.render()
    ren.render()
    s1 = ren.lighting()
    assert [round(float(x), 6) for x in s1.direction] == [0.6, 0.0, 0.8] and s1.is_reference == 0
    assert (s1.intensity, s1.ambient, s1.diffuse, s1.specular, s1.shininess) == (1.25, 0.25, 0.75, 0.5, 12.0)
    frame = hip_frame(ovr, ren)[0]
    inf, nan = float("inf"), float("nan")
    for bad in (lambda: ren.set_light_direction((0, 0, 0)), lambda: ren.set_light_direction((nan, 0, 1)), lambda: ren.set_light_direction((inf, 0, 1)),
                lambda: ren.set_light_direction((1e-30, 0, 0)), lambda: ren.set_light_direction((0, 0, 1), -1.0), lambda: ren.set_light_direction((0, 0, 1), nan),
                lambda: ren.set_material(-0.1, 0.5, 0, 0), lambda: ren.set_material(0.5, nan, 0, 0), lambda: ren.set_material(0.5, 0.5, inf, 0),
                lambda: ren.set_material(0.5, 0.5, 0.1, -1.0), lambda: ren.set_mat_specular(-2.0), lambda: ren.set_light_intensity(inf)):
        with pytest.raises(RuntimeError, match="ovr_hip_set_light|ovr_hip_set_material"):
            bad()
    ren.commit()                                     # nothing was queued by the refused calls
    ren.render()
    assert ren.stats().frame_index == 3              # ... so nothing was reset
    s2 = ren.lighting()
    assert list(s2.direction) == list(s1.direction) and (s2.intensity, s2.ambient, s2.diffuse, s2.specular, s2.shininess) == (1.25, 0.25, 0.75, 0.5, 12.0)
    assert np.allclose(hip_frame(ovr, ren)[0], frame, atol=1e-6)
    # the angle state: setting one angle keeps the other, starting from the literal's own angles
    ren2 = hip_setup(ovr, hip_renderer_factory(), case)
    ren2.set_light_theta(30.0)
    ren2.commit()
    phi_lit = lighting.angles_of(lighting.LITERAL_LIGHT)[0]
    assert np.array_equal(np.array(list(ren2.lighting().direction), F), lighting.normalize(lighting.direction_from_angles(phi_lit, 30.0)))
    ren2.set_light_phi(45.0)
    ren2.commit()
    assert np.array_equal(np.array(list(ren2.lighting().direction), F), lighting.normalize(lighting.direction_from_angles(45.0, 30.0)))
    ren.close(); ren2.close()


def test_a_light_change_voids_the_tuners_measurement(ovr, oracle, hip_renderer_factory):
    """as tests/test_round4_gpu.py::test_a_measured_layout_does_not_outlive_its_view for the camera: shadow rays change their length with the light, so what
    was measured under the old one does not outlive it - the next frame is the first of a configuration again (tuning 0), also in the middle of a probe"""
    case = make_case(ovr, oracle, n=48, tf="dense", cam="front", size=(96, 64), shading=2, rate=2.0)
    ren = hip_renderer_factory()
    ren.set_volume_layouts(2)
    hip_setup(ovr, ren, case)
    seen = []
    for _ in range(14):
        ren.render()
        seen.append(ren.stats().tuning)
    assert seen[-1] == 2 and 1 in seen, seen
    ren.set_light_direction((0.0, 1.0, 0.2))
    ren.commit()
    ren.render()
    assert ren.stats().tuning == 0
    for _ in range(4):                      # ... and it measures again
        ren.render()
        if ren.stats().tuning == 1:
            break
    assert ren.stats().tuning == 1
    ren.set_material(*SPECULAR)             # during the probe
    ren.commit()
    ren.render()
    assert ren.stats().tuning == 0
    seen = []
    for _ in range(13):
        ren.render()
        seen.append(ren.stats().tuning)
    assert seen[-1] == 2 and 1 in seen, seen
    os.environ["OVR_HIP_TUNE"] = "0"
    try:
        plain = hip_renderer_factory()
    finally:
        del os.environ["OVR_HIP_TUNE"]
    hip_setup(ovr, plain, case)
    plain.set_light_direction((0.0, 1.0, 0.2)); plain.set_material(*SPECULAR); plain.commit(); plain.render()
    assert np.array_equal(hip_frame(ovr, ren)[0].view(np.uint32), hip_frame(ovr, plain)[0].view(np.uint32))
    ren.close(); plain.close()


# ---- 7. the plugin -----------------------------------------------------------------------------------------------------------------------------------

def test_renderbatch_light_and_material_variables(tmp_path, ovr, oracle, hip_renderer_factory):
    if not (os.path.exists(RENDERBATCH) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/renderbatch or plugin/libdevice_hip.so missing: they are built by __graft_entry__.build() where the reference tree is present and travel with the snapshot")
    from PIL import Image
    n, W, H = 40, 96, 64
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("bumps", 256, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.25)
    env0 = dict(os.environ)
    env0["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env0.get("LD_LIBRARY_PATH", "")])
    for k in ("OVR_HIP_LIGHT", "OVR_HIP_MATERIAL", "OVR_HIP_QUIET"):
        env0.pop(k, None)

    def batch(tag, **extra):
        out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / tag)],
                             env=dict(env0, **extra), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        return open(str(tmp_path / f"{tag}000000.png"), "rb").read(), np.asarray(Image.open(str(tmp_path / f"{tag}000000.png")).convert("RGBA")), out.stderr

    plain_bytes, plain, err = batch("plain")
    assert "[hip] light:" not in err and "[hip] material:" not in err
    # the reference state spelled out in the variables is the frame without them, byte for byte
    same_bytes, _, err = batch("same", OVR_HIP_MATERIAL="0.5,0.5,0,0", OVR_HIP_LIGHT="%.9g,%.9g,1" % ovr.lighting.angles_of(ovr.lighting.LITERAL_LIGHT))
    assert "[hip] light: phi" in err and "[hip] material: ambient 0.5" in err
    lit_bytes, lit, err = batch("lit", OVR_HIP_LIGHT="60,200,1.5", OVR_HIP_MATERIAL="0.6,0.9,0.4,40")
    _, _, err_quiet = batch("quiet", OVR_HIP_LIGHT="60,200,1.5", OVR_HIP_MATERIAL="0.6,0.9,0.4,40", OVR_HIP_QUIET="1")
    assert "[hip] light" not in err_quiet and "[hip] material" not in err_quiet

    def host(setup):
        scene, camera = ovr.vidi3d.scene_from_file(scene_path)
        ren = hip_renderer_factory()
        ren.set_fbsize((W, H))
        ren.set_frame_accumulation(True)
        ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
        ren.init(scene, camera)
        ren.set_camera(camera.eye, camera.at, camera.up)   # fovy 60 (renderer.h:149-152)
        setup(ren)
        ren.commit()
        ren.render()
        return oracle.rgba8(hip_frame(ovr, ren)[0], flip=True).reshape(H, W, 4)

    def app_sliders(ren):
        ren.set_light_phi(60.0); ren.set_light_theta(200.0); ren.set_light_intensity(1.5)
        ren.set_mat_ambient(0.6); ren.set_mat_diffuse(0.9); ren.set_mat_specular(0.4); ren.set_mat_shininess(40.0)

    want_plain, want_lit = host(lambda r: None), host(app_sliders)
    assert np.abs(plain.astype(int) - want_plain.astype(int)).max() <= 1
    assert np.abs(lit.astype(int) - want_lit.astype(int)).max() <= 1
    assert np.abs(lit.astype(int) - plain.astype(int)).max() > 20
    # the angles of the literal are not the literal: the direction differs in its last bits, the 8-bit frame hardly
    _, same, _ = batch("same2", OVR_HIP_MATERIAL="0.5,0.5,0,0")
    assert open(str(tmp_path / "same2000000.png"), "rb").read() == plain_bytes
    assert np.abs(np.asarray(Image.open(str(tmp_path / "same000000.png")).convert("RGBA")).astype(int) - plain.astype(int)).max() <= 1


# ---- the oracle comparisons and the shade function once more, with equality ----------------------------------------------------------------------

def test_lighting_is_exact_under_the_exact_parity_build():
    """started the way tests/test_parity_exact_gpu.py starts its children: the exact-parity build of the kernels, the oracle in its "det" mode, helpers.compare =
    equality of every float.  Every light direction's frame (both layers, every counter, the shadow count included), the half material's frame and
    ovr_hip_shade_floats against lighting.py: bit for bit."""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "vs_oracle or vs_model"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    import re
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) >= 34 and "failed" not in out.stdout.splitlines()[-1], tail
