"""The depth limit on the GPU (include/ovr_hip.h ovr_hip_set_max_depth): pinned from one side by frames of the SAME build, bit for bit,
counters and gradient layer included - with no surface anywhere (+inf, NaN, values at or above every t1) the frame is the same state's frame without the limit,
for every voxel type and addressing mode; with depth = the clipped ray's exit under a clip box that removes only the far side the frame WITHOUT the clip box
is the clipped frame without the limit (which pins the cut, the shortened last step and the image's indexing); a surface in front gives a zero frame without a
sample; depth on a step boundary takes exactly k steps, one float above k + 1 - and everywhere else by the numpy model open-volume-renderer_amd/max_depth.py,
which tests/test_max_depth_model.py pins to the unmodified oracle.
"Bits" are float32 bit patterns.  Against the model the product build meets helpers.compare's float bar: its opacity correction goes through v_exp_f32 /
v_log_f32 and its normals through v_rsq_f32, so a ray with a loop test within 1e-5 of the termination threshold may take a step more or less, and a step whose
corrected opacity is at most 2^-22 may or may not count as shaded.  The exact-parity library (test_exact_under_the_exact_parity_build starts the model
comparisons with it) gives the model's bits and counters."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gradient_opacity_cases as GC
import max_depth_cases as MC
import preintegration_cases as QC
import projection_cases as PC
import signed_cases as SG
from helpers import EXACT_RUN, compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
F = np.float32
INF = float("inf")
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
TOL = 2e-4   # helpers.compare's float bar
# every voxel type under the modes 0 ... 3; the row loads (mode 4) where the layout has them: test_gradient_opacity_gpu.py's matrix
MATRIX = [(d, am) for d in QC.DTYPES for am in SG.ADDRESSING if am != "rows" or np.dtype(d).itemsize <= 2]
_IDS = [f"{np.dtype(d).name}-{am}" for d, am in MATRIX]
_models = {}


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, tf=MC.TF, cam=MC.CAMERA, rate=MC.RATE, shading=0, spp=1, size=PC.SIZE, volume_kind=MC.VOLUME, tfn=None):
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


def _limit(ren, image, active=None):
    """set the image (None: off), commit, and hold the getter to it"""
    ren.set_max_depth(image)
    ren.commit()
    g = ren.get_max_depth()
    on = image is not None
    assert g.mode == int(on) and g.active == (int(on) if active is None else active), (g.mode, g.active)
    assert (g.width, g.height) == ((image.shape[1], image.shape[0]) if on else (0, 0)), (g.width, g.height)
    return g


def _ortho(ovr, eye=MC.ORTHO_EYE, at=MC.CENTRE, height=MC.ORTHO_HEIGHT):
    return ovr.Camera(eye, at, (0.0, 1.0, 0.0), orthographic_height=height)


def _intervals(ren):
    """(t0, t1, hit), each (H, W), of the pixel-centre rays under the committed camera, volume and clip box: the device entries, pinned equal to the model's"""
    org, d = ren.camera_rays()
    h, w = org.shape[:2]
    t0, t1, hit = ren.clip_intervals(org.reshape(-1, 3), d.reshape(-1, 3))
    return t0.reshape(h, w), t1.reshape(h, w), hit.reshape(h, w)


def _lit(ren):
    ren.set_light_direction(MC.LIGHT, MC.INTENSITY)
    ren.set_material(*MC.MATERIAL)


# ---- 1. no surface: the same renderer's frame without the limit, in the product build ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_no_surface_gives_the_frame_without_the_limit(ovr, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = QC.volume("smooth", dtype)
    for shading in (0, 1):
        for cam in ("oblique", "axis", "orthographic"):
            case = _case(ovr, vol, tf="dense", cam="oblique" if cam == "orthographic" else cam, rate=1.0, shading=shading)
            ren = hip_setup(ovr, hip_renderer_factory(), case)
            if cam == "orthographic":
                ren.set_camera(_ortho(ovr))
            for rate, clip in ((1.0, None), (2.7, None), (0.5, MC.CLIP)):
                ren.set_volume_sampling_rate(rate)
                ren.set_clip_box(*clip) if clip else ren.set_clip_box(None)
                _limit(ren, None)
                off = _render(ovr, ren)
                _, t1, hit = _intervals(ren)
                for name, image in MC.no_surface_images(PC.SIZE, float(t1[hit].max())).items():
                    _limit(ren, image)
                    on = _render(ovr, ren)
                    tag = (np.dtype(dtype).name, am, shading, cam, rate, clip is not None, name)
                    _same_frame(on, off, tag)
                    _own_stats(on[2], tag)
                assert off[2].samples > 500 and off[2].shaded_samples > 300 and (off[0][..., 3] > 0.3).sum() > 100 and off[1].any() == (shading == 1), (cam, rate, off[2].samples)
            ren.close()


# ---- 2. depth = crop ---------------------------------------------------------------------------------------------------------------------------------------

def _crop_depth(ren, tag):
    """depth = where(hit_clip, t1_clip, 0) of the pixel-centre rays, from the device entries (ovr_hip_camera_rays, ovr_hip_clip_intervals)"""
    ren.set_clip_box(None)
    ren.commit()
    t0, t1, hit = _intervals(ren)
    ren.set_clip_box(*MC.FAR_CLIP)
    ren.commit()
    c0, c1, chit = _intervals(ren)
    # the precondition, on the CPU first: the box removes only the far side - a ray that hits under the clip has the unclipped entry and leaves no later
    assert (hit | ~chit).all() and _same(c0[chit], t0[chit]) and (c1[chit] <= t1[chit]).all() and (c1[chit] < t1[chit]).sum() > 100 and chit.sum() > 150, tag
    return np.where(chit, c1, F(0)).astype(F)


def _crop_pair(ovr, ren, depth):
    """the clipped frame without the limit, then - the clip box switched off - the frame limited to the clipped rays' exits"""
    ren.set_clip_box(*MC.FAR_CLIP)
    _limit(ren, None)
    clipped = _render(ovr, ren)
    ren.set_clip_box(None)
    _limit(ren, depth)
    limited = _render(ovr, ren)
    return clipped, limited


@pytest.mark.parametrize("orthographic", (False, True), ids=("perspective", "orthographic"))
@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
@pytest.mark.parametrize("size", MC.CROP_SIZES, ids=lambda s: "%dx%d" % s)
def test_depth_equal_to_the_clipped_exit_gives_the_clipped_frame(ovr, hip_renderer_factory, size, shading, orthographic):
    vol = QC.volume("smooth", np.float32)
    case = _case(ovr, vol, tf="dense", cam="oblique", size=size, shading=shading)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    if orthographic:
        ren.set_camera(_ortho(ovr))
    for rate in (1.0, 2.7):
        ren.set_volume_sampling_rate(rate)
        tag = (size, shading, orthographic, rate)
        clipped, limited = _crop_pair(ovr, ren, _crop_depth(ren, tag))
        _same_frame(limited, clipped, tag)
        _own_stats(limited[2], tag)
        assert clipped[2].shaded_samples > 500 and (clipped[0][..., 3] > 0.3).sum() > 50 and clipped[1].any() == (shading == 1), tag
    ren.close()


@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_a_device_group_of_three_gives_the_single_renderers_frames(ovr, hip_renderer_factory, shading):
    """the crop identity and the committed plane on a group: every member holds the whole image and indexes it by the full frame's pixel index"""
    size = MC.CROP_SIZES[1]
    case = _case(ovr, QC.volume("smooth", np.float32), tf="dense", cam="oblique", size=size, shading=shading)
    single = hip_setup(ovr, hip_renderer_factory(), case)
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        hip_setup(ovr, group, case)
        depth = _crop_depth(single, ("single", shading))
        clipped, limited = _crop_pair(ovr, single, depth)
        g_clipped, g_limited = _crop_pair(ovr, group, depth)
        _same_frame(limited, clipped, ("single", shading))
        for g, whole, name in ((g_clipped, clipped, "clipped"), (g_limited, limited, "limited")):
            assert _same(g[0], whole[0]) and _same(g[1], whole[1]), (name, shading)
            assert (g[2].rays, g[2].samples, g[2].shaded_samples, g[2].active_pixels) == (whole[2].rays, whole[2].samples, whole[2].shaded_samples, whole[2].active_pixels), (name, shading)
        image = MC.plane_image(size, (52.0, 0.45, 0.5))
        for r in (single, group):
            _limit(r, image)
        a, b = _render(ovr, single), _render(ovr, group)
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and (a[2].samples, a[2].shaded_samples) == (b[2].samples, b[2].shaded_samples) and a[2].samples > 500
        c, back = group.get_max_depth(values=True)
        assert (c.mode, c.active, c.width, c.height) == (1, 1, size[0], size[1]) and _same(back, image)
        with pytest.raises(ValueError):
            group.set_max_depth(image.reshape(-1), size=(0, size[1]))
    finally:
        group.close()
    single.close()


# ---- 3. the surface in front ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_a_surface_in_front_gives_a_zero_frame(ovr, hip_renderer_factory, shading):
    case = _case(ovr, QC.volume("smooth", np.float32), tf="dense", cam="oblique", shading=shading)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    off = _render(ovr, ren)
    t0, _, hit = _intervals(ren)
    h, w = PC.SIZE[::-1]
    for name, image in (("zero", np.zeros((h, w), F)), ("t0", np.where(hit, t0, F(0)).astype(F)), ("negative", np.full((h, w), -3.5, F)), ("-inf", np.full((h, w), -np.inf, F))):
        _limit(ren, image)
        got = _render(ovr, ren)
        assert not got[0].any() and not got[1].any() and got[2].samples == 0 and got[2].shaded_samples == 0 and got[2].rays == off[2].rays == w * h, (name, shading, got[2].samples)
        _own_stats(got[2], (name, shading))
    assert hit.sum() > 300 and off[2].samples > 500
    ren.close()


# ---- 4. the step boundary ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shade", (0, 1), ids=("none", "gradient"))
def test_depth_on_a_step_boundary_takes_exactly_k_steps(ovr, hip_renderer_factory, shade):
    vol, colors, alphas, vr = MC.ramp_volume_and_tables(ovr)
    case = _case(ovr, vol, cam=((-14.0, 21.0, -17.0), (8.0, 8.0, 8.0), (0.0, 1.0, 0.0)), rate=1.0, tfn=(colors, alphas, vr))
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    org, d = GC.dyadic_rays()
    t0, t1, hit = ren.clip_intervals(org, d)
    assert hit.all()
    whole = ren.max_depth_rays(org, d, np.full(len(org), np.inf, F), shade)
    assert _same(whole[1], t1) and _same(whole[2], t1)      # no surface: the cut is t1, and the rays (none saturates) run to it
    for k in MC.STEP_KS:
        z = (t0 + F(k)).astype(F)
        assert (z.astype(np.float64) == t0.astype(np.float64) + k).all()
        long = whole[0] > k
        steps, tc, tx, shaded, rgba = ren.max_depth_rays(org, d, z, shade)
        above = ren.max_depth_rays(org, d, np.nextafter(z, F(np.inf)), shade)
        assert long.sum() > 30 and (steps[long] == k).all() and (above[0][long] == k + 1).all(), (k, steps[long], above[0][long])
        assert _same(tc[long], z[long]) and _same(tx[long], z[long]) and (rgba[long, 3] < 0.9999).all() and (rgba[long, 3] > 0).sum() > 20
    ren.close()


# ---- 5. ovr_hip_max_depth_floats against the model -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_max_depth_floats_vs_model(ovr, hip_renderer_factory, dtype):
    M = ovr.max_depth
    org, d, z = MC.seeded_rays()
    vol = QC.volume(MC.VOLUME, dtype)
    case = _case(ovr, vol)
    ct, at, tfr = _tables(ovr, case)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _lit(ren)
    ren.commit()
    cam_pos = _basis(ren)[0]
    for shade in (0, 1):
        want = M.rays(vol, org, d, z, MC.RATE, ct, at, tfr, shading=shade, light=MC.LIGHT, intensity=MC.INTENSITY, material=MC.MATERIAL, cam_pos=cam_pos, border=MC.BORDER)
        steps, tc, tx, shaded, rgba = ren.max_depth_rays(org, d, z, shade)
        tag = (np.dtype(dtype).name, shade)
        miss = ~want["rays_hit"]
        print(tag, "hit", int((~miss).sum()), "cut inside", int((want["rays_hit"] & (want["tc"] < want["t1"]) & (want["tc"] > want["t0"])).sum()), "borderline", int(want["borderline"].sum()),
              "borderline steps", int(want["borderline_steps"].sum()), "max |rgba - model|", float(np.abs(rgba - want["rgba"]).max()), "steps differ", int((steps != want["steps"]).sum()),
              "shaded differ", int((shaded != want["shaded"]).sum()))
        assert miss.sum() > 100 and not rgba[miss].any() and (steps[miss] == 0).all() and not tx[miss].any() and not tc[miss].any(), tag
        assert _same(tc, want["tc"]), tag      # the cut is exact in both builds
        if EXACT_RUN:
            assert np.array_equal(steps, want["steps"]) and np.array_equal(shaded, want["shaded"]) and _same(tx, want["tx"]), tag
            assert _same(rgba, want["rgba"]), (tag, float(np.abs(rgba - want["rgba"]).max()))
        else:
            counted = ~want["borderline"]      # a ray's step count hangs on the last bit of the pow wherever a loop test was borderline
            assert counted.sum() > 1800, tag
            assert np.array_equal(steps[counted], want["steps"][counted]) and _same(tx[counted], want["tx"][counted]), tag
            assert (np.abs(shaded - want["shaded"])[counted] <= want["borderline_steps"][counted]).all(), tag
            assert not np.isnan(rgba).any() and np.abs(rgba - want["rgba"])[counted].max() <= TOL, (tag, float(np.abs(rgba - want["rgba"])[counted].max()))
        inside = want["rays_hit"] & (want["tc"] < want["t1"]) & (want["tc"] > want["t0"])
        assert (steps > 0).sum() > 1200 and inside.sum() > 800 and (rgba[:, 3] >= 0.9999).sum() > 50 and (want["rays_hit"] & (want["tc"] <= want["t0"])).sum() > 100
    ren.close()


# ---- 6. frames against the model -----------------------------------------------------------------------------------------------------------------------------------

def _check_frame(oracle, got, want, tag):
    rgba, layer, st = got
    ref, ref_layer, cnt = want
    _own_stats(st, tag)
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"], tag
    print(tag, "samples", st.samples, cnt["samples"], "shaded", st.shaded_samples, cnt["shaded"], "hinge", cnt["hinge"], "borderline steps", cnt["borderline_steps"], "borderline pixels",
          int(cnt["borderline"].sum()), "max |rgba - model|", float(np.abs(rgba - ref).max()), "max |layer - model|", float(np.abs(layer - ref_layer).max()))
    if EXACT_RUN:
        assert _same(rgba, ref) and _same(layer, ref_layer), (tag, float(np.abs(rgba - ref).max()), float(np.abs(layer - ref_layer).max()))
        assert st.samples == cnt["samples"] and st.shaded_samples == cnt["shaded"], (tag, st.samples, st.shaded_samples, cnt["samples"], cnt["shaded"])
        return
    # the product build: the pixels the model marks borderline are left out (the model test holds them under MC.BORDER_CAP of the hit rays)
    keep = ~cnt["borderline"]
    compare(oracle, np.where(keep[..., None], rgba, ref), ref, TOL, name=str(tag))
    assert not np.isnan(layer).any() and np.abs(layer - ref_layer)[keep].max() <= TOL, (tag, float(np.abs(layer - ref_layer)[keep].max()))
    assert abs(int(st.samples) - cnt["samples"]) <= cnt["hinge"], (tag, st.samples, cnt["samples"], cnt["hinge"])
    assert abs(int(st.shaded_samples) - cnt["shaded"]) <= cnt["hinge"] + cnt["borderline_steps"], (tag, st.shaded_samples, cnt["shaded"], cnt["hinge"], cnt["borderline_steps"])


def _model(ovr, ren, case, image, key=None, **kw):
    if key is not None and key in _models:
        return _models[key]
    ct, at, tfr = _tables(ovr, case)
    out = ovr.max_depth.frame(case["vol"], _basis(ren), case["size"], image, case["rate"], ct, at, tfr, shading=case["shading"], light=MC.LIGHT, intensity=MC.INTENSITY, material=MC.MATERIAL, **kw)
    if key is not None:
        _models[key] = out
    return out


@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, shading, dtype):
    """the committed case - a specular material under a light of its own, the tilted plane with its disc of +inf and its patch of NaN - as a perspective frame,
    then clipped under the orthographic camera"""
    vol = QC.volume(MC.VOLUME, dtype)
    nz, ny, nx = vol.shape
    name = np.dtype(dtype).name
    case = _case(ovr, vol, shading=shading)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _lit(ren)
    ren.commit()
    off = _render(ovr, ren)
    image = MC.plane_image()
    _limit(ren, image)
    got = _render(ovr, ren)
    _check_frame(oracle, got, _model(ovr, ren, case, image, key=("frame", name, shading)), (name, shading, "perspective"))
    free = ~np.isfinite(image)
    assert _same(got[0][free], off[0][free]) and not _same(got[0], off[0]) and got[2].samples < off[2].samples      # no surface there: the march's pixels
    assert (got[0][..., 3] >= 0.9999).sum() >= 30 and ((got[0][..., 3] > 0) & (got[0][..., 3] < 0.9999)).sum() >= 100 and got[1].any() == (shading == 1)
    ren.set_camera(_ortho(ovr))
    ren.set_clip_box(*MC.CLIP)
    image = MC.plane_image(PC.SIZE, MC.ORTHO_PLANE)
    _limit(ren, image)
    box = ovr.clipping.object_box(*MC.CLIP, *ovr.clipping.volume_constants((nx, ny, nz)))
    got = _render(ovr, ren)
    _check_frame(oracle, got, _model(ovr, ren, case, image, key=("ortho", name, shading), clip=box, camera_kind=ovr.camera.ORTHOGRAPHIC), (name, shading, "orthographic, clipped"))
    assert got[2].shaded_samples > 300
    ren.close()


@pytest.mark.parametrize("shading", (0, 1), ids=("none", "gradient"))
def test_accumulation_spp_and_jitter(ovr, oracle, hip_renderer_factory, shading):
    """every sample of a pixel (spp 3, blue-noise jitter) takes the pixel's depth"""
    vol = QC.volume(MC.VOLUME, np.float32)
    case = _case(ovr, vol, spp=3, shading=shading)
    noise = np.random.default_rng(77).random((16, 16, 64)).astype(F)
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    hip_setup(ovr, ren, case, accumulate=True)
    _lit(ren)
    image = MC.plane_image()
    _limit(ren, image)
    one = _render(ovr, ren)
    want1 = _model(ovr, ren, case, image, spp=3, noise=noise, frame_index=1)
    _check_frame(oracle, one, want1, ("spp 3, frame 1", shading))
    two = _render(ovr, ren)
    want2 = _model(ovr, ren, case, image, spp=3, noise=noise, frame_index=2)
    assert two[2].frame_index == 2 and not _same(want2[0], want1[0])
    # the accumulated frame: (A1 + A2) / 2 per channel, as write_pixel forms it
    acc = ((want1[0] + want2[0]).astype(F) / F(2)).astype(F)
    if EXACT_RUN:
        assert _same(two[0], acc) and two[2].samples == want2[2]["samples"]
    else:
        keep = ~(want1[2]["borderline"] | want2[2]["borderline"])
        compare(oracle, np.where(keep[..., None], two[0], acc), acc, TOL, name="accumulated")
        assert abs(int(two[2].samples) - want2[2]["samples"]) <= want2[2]["hinge"] and two[2].rays == want2[2]["rays"]
    ren.close()


# ---- 7. state -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_off_image_off_and_the_accumulation(ovr, hip_renderer_factory):
    vol = QC.volume(MC.VOLUME, np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    first = _render(ovr, ren)
    g = ren.get_max_depth()
    assert (g.mode, g.active, g.width, g.height) == (0, 0, 0, 0) and first[2].frame_index == 1 and ren.get_max_depth(values=True)[1] is None
    assert _render(ovr, ren)[2].frame_index == 2
    image = MC.plane_image()
    ren.set_max_depth(image)
    assert ren.get_max_depth().mode == 0 and _render(ovr, ren)[2].frame_index == 3      # queued: nothing changes before the commit
    _limit(ren, image)
    assert _same(ren.get_max_depth(values=True)[1], image)      # NaN payloads and infinities included
    cut = _render(ovr, ren)
    assert cut[2].frame_index == 1 and not _same(cut[0], first[0]) and 0 < cut[2].samples < first[2].samples
    assert _render(ovr, ren)[2].frame_index == 2
    _limit(ren, image)      # the same image again: still a call - contents are not compared, the accumulation starts over
    again = _render(ovr, ren)
    _same_frame(again, cut, "the same image again")
    assert again[2].frame_index == 1
    flat = np.full_like(image, 66.0)
    ren.set_max_depth(flat.reshape(-1), size=PC.SIZE)      # a flat array with its size; the renderer keeps its own copy
    flat[:] = 0.0
    ren.commit()
    assert (ren.get_max_depth(values=True)[1] == 66.0).all() and _render(ovr, ren)[2].samples != cut[2].samples
    _limit(ren, None)
    back = _render(ovr, ren)
    _same_frame(back, first, "off -> image -> off", COUNTERS + ("pipeline",))      # (not `layout`: a replica built in the background since the first frame may draw the later march)
    assert back[2].frame_index == 1
    # EINVAL: validated before anything changes (ValueError where the ABI says EINVAL)
    lib = ovr._lib.load()
    for w, h in ((0, 28), (40, 0), (-40, 28), (65536, 32768), (2 ** 31 - 1, 2)):
        assert lib.ovr_hip_set_max_depth(ren._h, image.ctypes.data, 0, w, h) == -1 and b"ovr_hip_set_max_depth" in lib.ovr_hip_last_error(), (w, h)
        with pytest.raises(ValueError, match="ovr_hip_set_max_depth"):
            ren.set_max_depth(image.reshape(-1), size=(w, h))
    assert lib.ovr_hip_set_max_depth(ren._h, image.ctypes.data, 2, 40, 28) == -1 and b"bad mem_kind" in lib.ovr_hip_last_error()
    ren.commit()
    assert ren.get_max_depth().mode == 0 and _render(ovr, ren)[2].frame_index == 2      # no call was recorded: the accumulation goes on
    # device memory: the same image from a device pointer
    import torch
    dev = torch.from_numpy(image).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert lib.ovr_hip_set_max_depth(ren._h, dev.data_ptr(), 1, 40, 28) == 0
    ren.commit()
    assert _same(ren.get_max_depth(values=True)[1], image)
    _same_frame(_render(ovr, ren), cut, "from device memory")
    ren.close()


def test_a_size_mismatch_keeps_the_image_and_draws_the_march(ovr, hip_renderer_factory):
    vol = QC.volume(MC.VOLUME, np.float32)
    case = _case(ovr, vol, shading=1)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    twin = hip_setup(ovr, hip_renderer_factory(), case)      # never hears of the limit
    image = MC.plane_image()
    _limit(ren, image)
    cut = _render(ovr, ren)
    assert not _same(cut[0], _render(ovr, twin)[0])
    for r in (ren, twin):
        r.set_fbsize((37, 23))
        r.commit()
    g = ren.get_max_depth()
    assert (g.mode, g.active, g.width, g.height) == (1, 0, 40, 28)
    _same_frame(_render(ovr, ren), _render(ovr, twin), "another framebuffer size: the march")
    small = MC.plane_image((37, 23))
    _limit(ren, small)      # an image of the new size is drawn
    assert _render(ovr, ren)[2].samples < _render(ovr, twin)[2].samples
    _limit(ren, image, active=0)      # ... and the old one is not
    _same_frame(_render(ovr, ren), _render(ovr, twin), "an image of another size: the march")
    for r in (ren, twin):
        r.set_fbsize(PC.SIZE)
        r.commit()
    assert ren.get_max_depth().active == 1
    _same_frame(_render(ovr, ren), cut, "the size set back: the limit resumes")
    twin.close()
    ren.close()


def test_the_other_frame_kinds_are_drawn_and_the_limit_resumes(ovr, hip_renderer_factory):
    vol = QC.volume(MC.VOLUME, np.float32)
    case = _case(ovr, vol, shading=1)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    twin = hip_setup(ovr, hip_renderer_factory(), case)      # never hears of the limit
    image = MC.plane_image()
    _limit(ren, image)
    cut = _render(ovr, ren)
    assert cut[1].any() and not _same(cut[0], _render(ovr, twin)[0])
    kinds = (("full shading", lambda r, on: r.set_shading(2 if on else 1)),
             ("slices", lambda r, on: r.set_slices([(MC.CENTRE, (0.0, 0.0, 1.0))] if on else None)),
             ("isovalues", lambda r, on: r.set_isosurfaces([0.5] if on else [])),
             ("projection", lambda r, on: r.set_projection(ovr.PROJECT_MAXIMUM if on else ovr.PROJECT_OFF)),
             ("gradient opacity", lambda r, on: r.set_gradient_opacity(1 if on else 0, *GC.RAMP_CASE)))
    for name, setter in kinds:
        for r in (ren, twin):
            setter(r, True)
            r.commit()
        g = ren.get_max_depth()
        assert (g.mode, g.active) == (1, 0), name
        if name == "gradient opacity":
            assert ren.get_gradient_opacity().active == 1      # its own rule and flag stay what they are
        a, b = _render(ovr, ren), _render(ovr, twin)
        _same_frame(a, b, name)      # (not `pipeline`: the automatic choice of the full-shaded march reads the frames a renderer drew before, and these two drew different ones)
        assert a[0].any() and not _same(a[0], cut[0]), name
        for r in (ren, twin):
            setter(r, False)
            r.commit()
        assert ren.get_max_depth().active == 1, name
        _same_frame(_render(ovr, ren), cut, name + " off: the limit resumes")
    # pre-integration: drawn under shading NONE alone, where it goes first
    for r in (ren, twin):
        r.set_preintegration(1)
        r.commit()
    assert ren.get_max_depth().active == 1 and ren.get_preintegration().active == 0
    _same_frame(_render(ovr, ren), cut, "pre-integration committed under GRADIENT: kept, the limit is drawn")
    for r in (ren, twin):
        r.set_shading(0)
        r.commit()
    g = ren.get_max_depth()
    assert (g.mode, g.active) == (1, 0) and ren.get_preintegration().active == 1
    _same_frame(_render(ovr, ren), _render(ovr, twin), "pre-integration under NONE")
    for r in (ren, twin):
        r.set_preintegration(0)
        r.commit()
    assert ren.get_max_depth().active == 1
    none = _render(ovr, ren)
    assert not none[1].any() and not _same(none[0], _render(ovr, twin)[0]) and none[2].samples == cut[2].samples      # (the steps do not depend on the shading)
    # errors of the known-answer entry; it needs no committed image
    import torch
    lib = ovr._lib.load()
    buf = torch.zeros(24, dtype=torch.float32, device=torch.device("cuda", 0))
    assert lib.ovr_hip_max_depth_floats(twin._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 0) == 0
    assert lib.ovr_hip_max_depth_floats(ren._h, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 0) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_max_depth_floats(ren._h, buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), 1, 0) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_max_depth_floats(ren._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 2) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    twin.close()
    ren.close()


# ---- 8. the exact-parity build -------------------------------------------------------------------------------------------------------------------------------------

def test_exact_under_the_exact_parity_build():
    """started the way tests/test_gradient_opacity_gpu.py starts its child: with the exact-parity build of the kernels the known-answer entry and the frames give
    the model's bits and counters for every voxel type"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
           "max_depth_floats_vs_model or test_frames_vs_model or accumulation_spp_and_jitter"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 3 * len(QC.DTYPES) + 2 and "failed" not in out.stdout.splitlines()[-1], tail
