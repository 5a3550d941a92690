"""Gradient opacity on the GPU (include/ovr_hip.h ovr_hip_set_gradient_opacity): pinned from one side by frames of the SAME renderer, bit
for bit and in the product build - under the neutral ramp (-1, 0) the frame is the OFF frame under shading NONE and GRADIENT (which is also the test that the
forward difference restated in ovr_hip_gradient_opacity.h is shade_request's), on a clipped ramp at dyadic positions it is the OFF frame under the halved alpha
table, over a constant volume it is zero, under a ramp steeper than hi it is the OFF frame - and everywhere else by the numpy model
open-volume-renderer_amd/gradient_opacity.py, which tests/test_gradient_opacity_model.py pins to the unmodified oracle.
"Bits" are float32 bit patterns.  Against the model the product build meets helpers.compare's float bar: its opacity correction goes through v_exp_f32 /
v_log_f32, its gradient multiplies with a stored reciprocal and its normals with v_rsq_f32, so a ray with a loop test within 1e-5 of the termination threshold
may take a step more or less, and a step whose (m - lo) * inv_ramp lies within 1e-4 of 0 may or may not have opacity.  The exact-parity library
(test_exact_under_the_exact_parity_build starts the model comparisons with it) gives the model's bits and counters."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gradient_opacity_cases as GC
import preintegration_cases as QC
import projection_cases as PC
import signed_cases as SG
from helpers import EXACT_RUN, compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
F = np.float32
INF = float("inf")
OFF, RAMP = 0, 1
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
TOL = 2e-4   # helpers.compare's float bar
# every voxel type under the modes 0 ... 3; the row loads (mode 4) where the layout has them
MATRIX = [(d, am) for d in QC.DTYPES for am in SG.ADDRESSING if am != "rows" or np.dtype(d).itemsize <= 2]
_IDS = [f"{np.dtype(d).name}-{am}" for d, am in MATRIX]
CLIP = ((5.5, -INF, 3.0), (27.0, 20.25, INF))
CENTRE = (20.0, 16.5, 9.0)
ORTHO_EYE = (-31.5, 44.25, -39.0)
_models = {}


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, tf=GC.TF, cam=GC.CAMERA, rate=GC.RATE, shading=0, spp=1, size=PC.SIZE, volume_kind=GC.VOLUME, tfn=None):
    colors, alphas, vr = QC.transfer_function(ovr, tf, vol.dtype, volume_kind) if tfn is None else tfn
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=PC.CAMERAS[cam] if isinstance(cam, str) else cam, size=size, shading=shading, rate=rate, spp=spp,
                convention=0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=PC.FOVY)


def _render(ovr, ren):
    ren.render()
    rgba, layer = hip_frame(ovr, ren)
    return rgba, layer, ren.stats()


def _basis(ren):
    c = ren.get_camera()
    return tuple(np.array(list(v), F) for v in (c.pos, c.dir, c.hor, c.ver))


def _tables(ovr, case):
    ct, at = PC.tables(case["colors"], case["alphas"])
    return ct, at, ovr.projection.normalized_range(case["vr"], case["vol"].dtype)


def _same_frame(a, b, tag, counters=COUNTERS):
    assert _same(a[0], b[0]) and _same(a[1], b[1]), (tag, float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))
    assert [getattr(a[2], k) for k in counters] == [getattr(b[2], k) for k in counters], (tag, [(k, getattr(a[2], k), getattr(b[2], k)) for k in counters])


def _own_stats(st, tag):
    assert st.skipped_samples == 0 and st.shadow_samples == 0 and st.skipped_shadow_samples == 0 and st.layout == 0 and st.pipeline == 1 and st.tuning == 0, tag
    assert st.skipping_kernels == 0, tag


def _switch(ren, mode, lo=0.0, hi=1.0, active=None):
    ren.set_gradient_opacity(mode, lo, hi)
    ren.commit()
    g = ren.get_gradient_opacity()
    assert g.mode == mode and g.active == (mode if active is None else active), (g.mode, g.active)
    return g


def _ortho(ovr, eye=ORTHO_EYE, at=CENTRE, height=40.0):
    return ovr.Camera(eye, at, (0.0, 1.0, 0.0), orthographic_height=height)


# ---- 1. the neutral ramp: the same renderer's OFF frame, in the product build --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_the_neutral_ramp_gives_the_off_frame(ovr, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = QC.volume("smooth", dtype)
    for shading in (0, 1):
        for cam in ("oblique", "axis", "orthographic"):
            case = _case(ovr, vol, tf="dense", cam="oblique" if cam == "orthographic" else cam, rate=1.0, shading=shading)
            ren = hip_setup(ovr, hip_renderer_factory(), case)
            if cam == "orthographic":
                ren.set_camera(_ortho(ovr))
            for rate, clip in ((1.0, None), (2.7, None), (0.5, CLIP)):
                ren.set_volume_sampling_rate(rate)
                ren.set_clip_box(*clip) if clip else ren.set_clip_box(None)
                _switch(ren, OFF)
                off = _render(ovr, ren)
                g = _switch(ren, RAMP, *GC.NEUTRAL)
                assert (g.lo, g.hi, g.inv_ramp) == (-1.0, 0.0, 1.0)
                on = _render(ovr, ren)
                tag = (np.dtype(dtype).name, am, shading, cam, rate, clip is not None)
                _same_frame(on, off, tag)
                _own_stats(on[2], tag)
                assert off[2].samples > 500 and off[2].shaded_samples > 300 and (off[0][..., 3] > 0.3).sum() > 100 and off[1].any() == (shading == 1), (tag, off[2].samples)
            ren.close()


# ---- 2. the halved table on a ramp ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_a_ramp_at_dyadic_positions_gives_the_off_frame_under_the_halved_table(ovr, hip_renderer_factory, shading):
    """the orthographic camera along +z over the 16^3 ramp, 16 x 16 pixels of 0.5 world units: the pixel centres are multiples of 0.25, every gradient is exactly
    (1/32, 0, 0), every w exactly 0.5 - and dims of 16 make the product's stored reciprocal exact"""
    vol = GC.x_ramp_volume()
    cam = ((8.0, 8.0, -20.0), (8.0, 8.0, 8.0), (0.0, 1.0, 0.0))
    frames = {}
    for half in (False, True):
        case = _case(ovr, vol, cam=cam, size=(16, 16), shading=shading, tfn=GC.ramp_tables(ovr, half))
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        ren.set_camera(_ortho(ovr, cam[0], cam[1], 8.0))
        ren.set_clip_box(*GC.RAMP_CLIP)
        for rate in (1.0, 2.0, 0.5):
            ren.set_volume_sampling_rate(rate)
            if half:
                _switch(ren, OFF)
            else:
                _switch(ren, RAMP, *GC.RAMP_HALF)
            frames[(half, rate)] = _render(ovr, ren)
        ren.close()
    for rate in (1.0, 2.0, 0.5):
        weighted, plain = frames[(False, rate)], frames[(True, rate)]
        _same_frame(weighted, plain, ("halved table", shading, rate))
        a = weighted[0][..., 3]
        print("rate", rate, "alpha", float(a.min()), "...", float(a.max()), "samples", weighted[2].samples)
        assert a.max() > 0.5 and weighted[2].samples == 256 * int(10 * rate) and weighted[2].shaded_samples > 0.8 * weighted[2].samples


# ---- 3. a constant volume; a ramp steeper than hi ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_constant_volume_gives_a_zero_frame(ovr, hip_renderer_factory, dtype):
    vol = QC.constant_volume(dtype)
    for shading in (0, 1):
        case = _case(ovr, vol, tf="dense", cam="oblique", shading=shading)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        fog = _render(ovr, ren)
        assert fog[2].shaded_samples == fog[2].samples > 500      # the plain march is opaque fog
        # the march of the same rays without early termination: the same colours over an alpha table of 1e-6 (nothing saturates, no macrocell is empty)
        clear = _case(ovr, vol, tf="dense", cam="oblique", shading=shading)
        clear["alphas"] = np.array(clear["alphas"], F).copy()
        clear["alphas"][1::2] = 1e-6
        twin = hip_setup(ovr, hip_renderer_factory(), clear)
        steps = _render(ovr, twin)[2]
        for lo, hi in ((0.0, 1.0), (0.02, 0.06)):
            _switch(ren, RAMP, lo, hi)
            got = _render(ovr, ren)
            tag = (np.dtype(dtype).name, shading, lo, hi)
            assert not got[0].any() and not got[1].any() and got[2].shaded_samples == 0, tag
            assert got[2].samples == steps.samples >= fog[2].samples and steps.skipped_samples == 0 and got[2].rays == fog[2].rays, (tag, got[2].samples, steps.samples, steps.skipped_samples)
            _own_stats(got[2], tag)
        twin.close()
        ren.close()


@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_a_ramp_steeper_than_hi_gives_the_off_frame(ovr, hip_renderer_factory, shading):
    vol = GC.x_ramp_volume()
    for cam in (((-14.0, 21.0, -17.0), (8.0, 8.0, 8.0), (0.0, 1.0, 0.0)), ((30.0, 3.0, 25.0), (8.0, 8.0, 8.0), (0.0, 1.0, 0.0))):
        case = _case(ovr, vol, cam=cam, rate=2.7, shading=shading, tfn=GC.ramp_tables(ovr))
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        ren.set_clip_box(*GC.RAMP_CLIP)
        _switch(ren, OFF)
        off = _render(ovr, ren)
        _switch(ren, RAMP, *GC.RAMP_SATURATED)
        _same_frame(_render(ovr, ren), off, ("saturated", shading, cam[0]))
        assert off[2].shaded_samples > 500 and (off[0][..., 3] > 0.3).sum() > 50
        ren.close()


# ---- 4. ovr_hip_gradient_opacity_floats against the model ---------------------------------------------------------------------------------------------------

def _seeded_rays(n=2400, seed=25):
    """world rays towards the 40 x 33 x 18 box from all around it; one in eight misses"""
    rng = np.random.default_rng(seed)
    dims = np.array(PC.DIMS[0], np.float64)
    target = rng.random((n, 3)) * dims
    target[::8] += 3.0 * dims      # misses
    v = rng.normal(size=(n, 3))
    org = 0.5 * dims + 70.0 * v / np.linalg.norm(v, axis=1)[:, None]
    d = target - org
    return org.astype(F), (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)


def _lit(ren):
    ren.set_light_direction(GC.LIGHT, GC.INTENSITY)
    ren.set_material(*GC.MATERIAL)


@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_gradient_opacity_floats_vs_model(ovr, hip_renderer_factory, dtype):
    G = ovr.gradient_opacity
    org, d = _seeded_rays()
    vol = QC.volume(GC.VOLUME, dtype)
    case = _case(ovr, vol)
    ct, at, tfr = _tables(ovr, case)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _lit(ren)
    _switch(ren, RAMP, *GC.RAMP_CASE)
    cam_pos = _basis(ren)[0]
    for shade in (0, 1):
        want = G.rays(vol, org, d, GC.RATE, ct, at, tfr, *GC.RAMP_CASE, shading=shade, light=GC.LIGHT, intensity=GC.INTENSITY, material=GC.MATERIAL, cam_pos=cam_pos,
                      border=GC.BORDER, w_border=GC.W_BORDER)
        steps, gradients, tx, shaded, rgba = ren.gradient_opacity_rays(org, d, shade)
        tag = (np.dtype(dtype).name, shade)
        miss = ~want["rays_hit"]
        print(tag, "hit", int((~miss).sum()), "borderline", int(want["borderline"].sum()), "w-borderline steps", int(want["w_borderline"].sum()), "max |rgba - model|",
              float(np.abs(rgba - want["rgba"]).max()), "steps differ", int((steps != want["steps"]).sum()), "gradients differ", int((gradients != want["gradients"]).sum()),
              "shaded differ", int((shaded != want["shaded"]).sum()))
        assert miss.sum() > 100 and not rgba[miss].any() and (steps[miss] == 0).all() and not tx[miss].any(), tag
        if EXACT_RUN:
            assert np.array_equal(steps, want["steps"]) and np.array_equal(gradients, want["gradients"]) and np.array_equal(shaded, want["shaded"]) and _same(tx, want["tx"]), tag
            assert _same(rgba, want["rgba"]), (tag, float(np.abs(rgba - want["rgba"]).max()))
        else:
            counted = ~want["borderline"]      # a ray's step count hangs on the last bit of the pow wherever a loop test was borderline
            assert counted.sum() > 1800, tag
            assert np.array_equal(steps[counted], want["steps"][counted]) and _same(tx[counted], want["tx"][counted]), tag
            assert np.array_equal(gradients[counted], want["gradients"][counted]), tag
            assert (np.abs(shaded - want["shaded"])[counted] <= want["w_borderline"][counted]).all(), tag
            assert not np.isnan(rgba).any() and np.abs(rgba - want["rgba"])[counted].max() <= TOL, (tag, float(np.abs(rgba - want["rgba"])[counted].max()))
        assert (steps > 0).sum() > 1500 and (want["w_min"] < 1).sum() > 1000 and (rgba[:, 3] >= 0.9999).sum() > 100
    ren.close()


# ---- 5. frames against the model under a non-neutral ramp ------------------------------------------------------------------------------------------------------

def _check_frame(oracle, got, want, tag):
    rgba, layer, st = got
    ref, ref_layer, cnt = want
    _own_stats(st, tag)
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"], tag
    print(tag, "samples", st.samples, cnt["samples"], "shaded", st.shaded_samples, cnt["shaded"], "hinge", cnt["hinge"], "w-borderline", cnt["w_borderline"], "borderline pixels",
          int(cnt["borderline"].sum()), "max |rgba - model|", float(np.abs(rgba - ref).max()), "max |layer - model|", float(np.abs(layer - ref_layer).max()))
    if EXACT_RUN:
        assert _same(rgba, ref) and _same(layer, ref_layer), (tag, float(np.abs(rgba - ref).max()), float(np.abs(layer - ref_layer).max()))
        assert st.samples == cnt["samples"] and st.shaded_samples == cnt["shaded"], (tag, st.samples, st.shaded_samples, cnt["samples"], cnt["shaded"])
        return
    compare(oracle, rgba, ref, TOL, name=str(tag))
    assert not np.isnan(layer).any() and np.abs(layer - ref_layer).max() <= TOL, (tag, float(np.abs(layer - ref_layer).max()))
    assert abs(int(st.samples) - cnt["samples"]) <= cnt["hinge"], (tag, st.samples, cnt["samples"], cnt["hinge"])
    assert abs(int(st.shaded_samples) - cnt["shaded"]) <= cnt["hinge"] + cnt["w_borderline"], (tag, st.shaded_samples, cnt["shaded"], cnt["hinge"], cnt["w_borderline"])


def _model(ovr, ren, case, key=None, **kw):
    if key is not None and key in _models:
        return _models[key]
    ct, at, tfr = _tables(ovr, case)
    out = ovr.gradient_opacity.frame(case["vol"], _basis(ren), case["size"], case["rate"], ct, at, tfr, *GC.RAMP_CASE, shading=case["shading"], light=GC.LIGHT, intensity=GC.INTENSITY,
                                     material=GC.MATERIAL, **kw)
    if key is not None:
        _models[key] = out
    return out


@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, shading, dtype):
    """the committed case - a specular material under a light of its own - as a perspective frame, then clipped under the orthographic camera"""
    vol = QC.volume(GC.VOLUME, dtype)
    nz, ny, nx = vol.shape
    name = np.dtype(dtype).name
    case = _case(ovr, vol, shading=shading)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _lit(ren)
    _switch(ren, RAMP, *GC.RAMP_CASE)
    got = _render(ovr, ren)
    _check_frame(oracle, got, _model(ovr, ren, case, key=("frame", name, shading)), (name, shading, "perspective"))
    assert (got[0][..., 3] >= 0.9999).sum() >= 100 and ((got[0][..., 3] > 0) & (got[0][..., 3] < 0.9999)).sum() >= 100 and got[1].any() == (shading == 1)
    ren.set_camera(_ortho(ovr))
    ren.set_clip_box(*CLIP)
    ren.commit()
    box = ovr.clipping.object_box(*CLIP, *ovr.clipping.volume_constants((nx, ny, nz)))
    got = _render(ovr, ren)
    _check_frame(oracle, got, _model(ovr, ren, case, key=("ortho", name, shading), clip=box, camera_kind=ovr.camera.ORTHOGRAPHIC), (name, shading, "orthographic, clipped"))
    assert got[2].shaded_samples > 300
    ren.close()


@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_accumulation_spp_and_jitter(ovr, oracle, hip_renderer_factory, shading):
    vol = QC.volume(GC.VOLUME, np.float32)
    case = _case(ovr, vol, spp=3, shading=shading)
    noise = np.random.default_rng(77).random((16, 16, 64)).astype(F)
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    hip_setup(ovr, ren, case, accumulate=True)
    _lit(ren)
    _switch(ren, RAMP, *GC.RAMP_CASE)
    one = _render(ovr, ren)
    want1 = _model(ovr, ren, case, spp=3, noise=noise, frame_index=1)
    _check_frame(oracle, one, want1, ("spp 3, frame 1", shading))
    two = _render(ovr, ren)
    want2 = _model(ovr, ren, case, spp=3, noise=noise, frame_index=2)
    assert two[2].frame_index == 2 and not _same(want2[0], want1[0])
    # the accumulated frame: (A1 + A2) / 2 per channel, as write_pixel forms it
    acc = ((want1[0] + want2[0]).astype(F) / F(2)).astype(F)
    if EXACT_RUN:
        assert _same(two[0], acc) and two[2].samples == want2[2]["samples"]
    else:
        compare(oracle, two[0], acc, TOL, name="accumulated")
        assert abs(int(two[2].samples) - want2[2]["samples"]) <= want2[2]["hinge"] and two[2].rays == want2[2]["rays"]
    ren.close()


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_off_ramp_off_and_the_accumulation(ovr, hip_renderer_factory):
    vol = QC.volume(GC.VOLUME, np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    first = _render(ovr, ren)
    g = ren.get_gradient_opacity()
    assert (g.mode, g.active, g.lo, g.hi, g.inv_ramp) == (OFF, 0, 0.0, 1.0, 1.0) and first[2].frame_index == 1
    assert _render(ovr, ren)[2].frame_index == 2
    g = _switch(ren, RAMP, *GC.RAMP_CASE)
    assert (F(g.lo), F(g.hi), F(g.inv_ramp)) == ovr.gradient_opacity.commit(RAMP, *GC.RAMP_CASE)[1:]
    ramp = _render(ovr, ren)
    assert ramp[2].frame_index == 1 and not _same(ramp[0], first[0]) and ramp[2].shaded_samples > 0 and ramp[2].samples >= first[2].samples
    assert _render(ovr, ren)[2].frame_index == 2
    _switch(ren, RAMP, *GC.RAMP_CASE)      # the same values again: still a call - the accumulation starts over
    again = _render(ovr, ren)
    _same_frame(again, ramp, "the same ramp again")
    assert again[2].frame_index == 1
    _switch(ren, OFF, 7.0, 3.0)             # OFF ignores the thresholds
    g = ren.get_gradient_opacity()
    assert (g.lo, g.hi, g.inv_ramp) == (0.0, 1.0, 1.0)
    back = _render(ovr, ren)
    _same_frame(back, first, "OFF -> RAMP -> OFF", COUNTERS + ("pipeline",))      # (not `layout`: a replica built in the background since the first frame may draw the later march)
    assert back[2].frame_index == 1
    for args in ((2, 0.0, 1.0), (-1, 0.0, 1.0), (RAMP, 1.0, 1.0), (RAMP, 2.0, 1.0), (RAMP, float("nan"), 1.0), (RAMP, 0.0, INF), (OFF, -INF, 0.0)):
        with pytest.raises(ValueError, match="ovr_hip_set_gradient_opacity"):      # refused values leave the state alone (ValueError where the ABI says EINVAL)
            ren.set_gradient_opacity(*args)
    ren.commit()
    assert ren.get_gradient_opacity().mode == OFF and _render(ovr, ren)[2].frame_index == 2      # no call was recorded: the accumulation goes on
    ren.close()


def test_the_other_frame_kinds_are_drawn_and_gradient_opacity_resumes(ovr, hip_renderer_factory):
    vol = QC.volume(GC.VOLUME, np.float32)
    case = _case(ovr, vol, shading=1)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    twin = hip_setup(ovr, hip_renderer_factory(), case)      # never hears of gradient opacity
    _switch(ren, RAMP, *GC.RAMP_CASE)
    ramp = _render(ovr, ren)
    assert ramp[1].any() and not _same(ramp[0], _render(ovr, twin)[0])
    kinds = (("full shading", lambda r, on: r.set_shading(2 if on else 1)),
             ("slices", lambda r, on: r.set_slices([(CENTRE, (0.0, 0.0, 1.0))] if on else None)),
             ("isovalues", lambda r, on: r.set_isosurfaces([0.5] if on else [])),
             ("projection", lambda r, on: r.set_projection(ovr.PROJECT_MAXIMUM if on else ovr.PROJECT_OFF)))
    for name, setter in kinds:
        for r in (ren, twin):
            setter(r, True)
            r.commit()
        g = ren.get_gradient_opacity()
        assert (g.mode, g.active) == (RAMP, 0), name
        a, b = _render(ovr, ren), _render(ovr, twin)
        _same_frame(a, b, name)      # (not `pipeline`: the automatic choice of the full-shaded march reads the frames a renderer drew before, and these two drew different ones)
        assert a[0].any() and not _same(a[0], ramp[0]), name
        for r in (ren, twin):
            setter(r, False)
            r.commit()
        assert ren.get_gradient_opacity().active == 1, name
        _same_frame(_render(ovr, ren), ramp, name + " off: gradient opacity resumes")
    # pre-integration: drawn under shading NONE alone, where it goes first
    for r in (ren, twin):
        r.set_preintegration(1)
        r.commit()
    assert ren.get_gradient_opacity().active == 1 and ren.get_preintegration().active == 0
    _same_frame(_render(ovr, ren), ramp, "pre-integration committed under GRADIENT: neither kept mode changes the frame kind")
    for r in (ren, twin):
        r.set_shading(0)
        r.commit()
    g = ren.get_gradient_opacity()
    assert (g.mode, g.active) == (RAMP, 0) and ren.get_preintegration().active == 1
    _same_frame(_render(ovr, ren), _render(ovr, twin), "pre-integration under NONE")
    for r in (ren, twin):
        r.set_preintegration(0)
        r.commit()
    assert ren.get_gradient_opacity().active == 1
    none = _render(ovr, ren)
    assert not none[1].any() and not _same(none[0], _render(ovr, twin)[0]) and none[2].shaded_samples == ramp[2].shaded_samples      # (the weight does not depend on the shading)
    # errors of the known-answer entry
    import torch
    lib = ovr._lib.load()
    buf = torch.zeros(24, dtype=torch.float32, device=torch.device("cuda", 0))
    assert lib.ovr_hip_gradient_opacity_floats(twin._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 0) < 0
    assert b"no gradient opacity is committed (ovr_hip_set_gradient_opacity)" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_gradient_opacity_floats(ren._h, None, buf.data_ptr(), buf.data_ptr(), 1, 0) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_gradient_opacity_floats(ren._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 2) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    twin.close()
    ren.close()


# ---- 7. a device group ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_a_device_group_of_three_gives_the_single_renderers_frame(ovr, hip_renderer_factory, shading):
    case = _case(ovr, QC.volume(GC.VOLUME, np.float32), size=(56, 40), shading=shading)

    def start(ren):
        hip_setup(ovr, ren, case)
        _lit(ren)
        ren.set_gradient_opacity(RAMP, *GC.RAMP_CASE)
        ren.commit()
        return ren

    single = start(hip_renderer_factory())
    whole = _render(ovr, single)
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        g = _render(ovr, start(group))
        c = group.get_gradient_opacity()
        assert _same(g[0], whole[0]) and _same(g[1], whole[1]) and (c.mode, c.active) == (RAMP, 1)
        assert (g[2].rays, g[2].samples, g[2].shaded_samples, g[2].active_pixels) == (whole[2].rays, whole[2].samples, whole[2].shaded_samples, whole[2].active_pixels)
        with pytest.raises(ValueError):
            group.set_gradient_opacity(RAMP, 1.0, 0.0)
    finally:
        group.close()
    assert whole[2].shaded_samples > 500
    single.close()


# ---- 8. the exact-parity build -------------------------------------------------------------------------------------------------------------------------------------

def test_exact_under_the_exact_parity_build():
    """started the way tests/test_preintegration_gpu.py starts its child: with the exact-parity build of the kernels the known-answer entry and the frames give the
    model's bits and counters for every voxel type"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
           "gradient_opacity_floats_vs_model or test_frames_vs_model or accumulation_spp_and_jitter"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 3 * len(QC.DTYPES) + 2 and "failed" not in out.stdout.splitlines()[-1], tail
