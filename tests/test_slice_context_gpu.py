"""The slice context on the GPU (include/ovr_hip.h ovr_hip_set_slice_context): pinned from both sides by frames of the SAME renderer - with
slices no ray meets the context frame is the SHADE_NONE march frame, with nothing in front (an all-zero alpha table, scale 0) it is the slice frame, bit for bit
and in the product build - and in between by the numpy model open-volume-renderer_amd/slice_context.py, which tests/test_slice_context_model.py pins to the
unmodified oracle and to the slice model.  "Bits" are float32 bit patterns.  The context's opacities go through the opacity correction's pow: the product
evaluates it with v_exp_f32 / v_log_f32, so against the model it meets helpers.compare's float bar, and a ray whose alpha before the slice lies within 1e-5 of
the termination threshold may fall on either side of it; the exact-parity library (test_exact_under_the_exact_parity_build starts this file with it) gives the
model's bits and counters for every type."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import projection_cases as PC
import signed_cases as SG
import slice_context_cases as CC
from helpers import EXACT_RUN, compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
F = np.float32
INF = float("inf")
OFF, FRONT = 0, 1
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
TOL = 2e-4   # helpers.compare's float bar
# every voxel type under the modes 0 ... 3; the row loads (mode 4) where the layout has them
MATRIX = [(d, am) for d in CC.DTYPES for am in SG.ADDRESSING if am != "rows" or np.dtype(d).itemsize <= 2]
_IDS = [f"{np.dtype(d).name}-{am}" for d, am in MATRIX]
CLIP = ((5.5, -INF, 3.0), (27.0, 20.25, INF))
_models = {}


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, tf="dense", cam=CC.CAMERA, rate=CC.RATE, shading=0, spp=1, size=PC.SIZE):
    colors, alphas, vr = CC.transfer_function(ovr, tf, vol.dtype)
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=PC.CAMERAS[cam], size=size, shading=shading, rate=rate, spp=spp, convention=0,
                spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=PC.FOVY)


def _render(ovr, ren):
    ren.render()
    rgba, layer = hip_frame(ovr, ren)
    return rgba, layer, ren.stats()


def _basis(ren):
    c = ren.get_camera()
    return tuple(np.array(list(v), F) for v in (c.pos, c.dir, c.hor, c.ver))


def _model(ovr, ren, case, slices, scale=1.0, key=None, **kw):
    """the model's frame; `key` caches it across the addressing modes (the frame does not depend on them)"""
    if key is not None and key in _models:
        return _models[key]
    ct, at = PC.tables(case["colors"], case["alphas"])
    out = ovr.slice_context.frame(case["vol"], _basis(ren), case["size"], case["rate"], slices, ct, at, ovr.projection.normalized_range(case["vr"], case["vol"].dtype),
                                  opacity_scale=scale, **kw)
    if key is not None:
        _models[key] = out
    return out


def _same_frame(a, b, tag, counters=COUNTERS):
    assert _same(a[0], b[0]) and _same(a[1], b[1]), (tag, float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))
    assert [getattr(a[2], k) for k in counters] == [getattr(b[2], k) for k in counters], (tag, [(k, getattr(a[2], k), getattr(b[2], k)) for k in counters])


def _context_stats(st, tag):
    assert st.skipped_samples == 0 and st.shadow_samples == 0 and st.skipped_shadow_samples == 0 and st.layout == 0 and st.pipeline == 1 and st.tuning == 0, tag
    assert st.skipping_kernels == 0, tag


def _check_frame(ovr, oracle, case, got, want, tag):
    """a context frame against the model's: bits and counters under the exact-parity library; in the product build the float bar on rgba, the layer exact
    outside the model's borderline pixels, `samples` within the samples that hang on a borderline termination"""
    rgba, layer, st = got
    ref, ref_layer, cnt = want
    _context_stats(st, tag)
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"], tag
    print(tag, "samples", st.samples, cnt["samples"], "shaded", st.shaded_samples, cnt["shaded"], "hinge", cnt["hinge"], "borderline pixels", int(cnt["borderline_front"].sum()), "of", int((ref_layer[..., 2] > 0).sum()), "composited",
          "max |rgba - model|", float(np.abs(rgba - ref).max()))
    if EXACT_RUN:
        assert _same(rgba, ref) and _same(layer, ref_layer), (tag, float(np.abs(rgba - ref).max()))
        assert st.samples == cnt["samples"] and st.shaded_samples == cnt["shaded"], (tag, st.samples, st.shaded_samples, cnt)
        return
    compare(oracle, rgba, ref, TOL, name=str(tag))
    keep = ~cnt["borderline_front"]     # (tests/test_slice_context_model.py caps their share for the committed case)
    eight_bit = np.dtype(case["vol"].dtype).itemsize == 1   # (the product normalises 8-bit voxels behind the filter: v meets the float bar, t_k and k are exact)
    if eight_bit:
        assert np.abs(layer[..., 0] - ref_layer[..., 0])[keep].max() <= TOL and _same(layer[..., 1:][keep], ref_layer[..., 1:][keep]), tag
    else:
        assert _same(layer[keep], ref_layer[keep]), (tag, int((_bits(layer) != _bits(ref_layer)).any(-1)[keep].sum()))
    assert abs(int(st.samples) - cnt["samples"]) <= cnt["hinge"] and abs(int(st.shaded_samples) - cnt["shaded"]) <= cnt["hinge"] + cnt["borderline_steps"], (tag, st.samples, cnt)


# ---- 1. no slice met: the same renderer's SHADE_NONE march, in the product build --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_unmet_slices_give_the_march_frame(ovr, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = CC.volume(dtype)
    for cam in sorted(PC.CAMERAS):
        case = _case(ovr, vol, cam=cam, rate=1.0)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        for rate, clip in ((1.0, None), (2.7, None), (CC.RATE, CLIP)):
            ren.set_volume_sampling_rate(rate)
            ren.set_clip_box(*clip) if clip else ren.set_clip_box(None)
            ren.set_slices(None)
            ren.set_slice_context(FRONT, 1.0)      # kept while no slice is committed: the march
            ren.commit()
            assert ren.slice_context().mode == FRONT and ren.slice_context().active == 0
            march = _render(ovr, ren)
            ren.set_slices(CC.NO_MEET)
            ren.commit()
            assert ren.slice_context().active == 1
            ctx = _render(ovr, ren)
            tag = (np.dtype(dtype).name, am, cam, rate, clip is not None)
            _same_frame(ctx, march, tag)
            _context_stats(ctx[2], tag)
            assert march[2].samples > 500 and march[2].shaded_samples > 300 and not march[1].any() and (clip or (march[0][..., 3] >= 0.9999).sum() > 20), (tag, march[2].samples)
            # and the plain slice frame of these slices is empty: the identity does not rest on the slices being ignored
            ren.set_slice_context(OFF)
            ren.commit()
            plain = _render(ovr, ren)
            assert not plain[0].any() and plain[2].samples == 0 and ren.slice_context().active == 0, tag
        ren.close()


def test_unmet_slices_give_the_march_frame_orthographic_and_shaded_state(ovr, hip_renderer_factory):
    """the orthographic twin; and the shading mode, the light and empty-space skipping are ignored: the context is the UNSHADED march whatever is committed"""
    vol = CC.volume(np.float32)
    case = _case(ovr, vol, rate=1.0)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_camera(ovr.Camera((-31.5, 44.25, -39.0), CC.CENTRE, (0.0, 1.0, 0.0), orthographic_height=40.0))
    ren.commit()
    march = _render(ovr, ren)
    ren.set_slices(CC.NO_MEET)
    ren.set_slice_context(FRONT, 1.0)
    ren.commit()
    ctx = _render(ovr, ren)
    _same_frame(ctx, march, "orthographic")
    assert march[2].samples > 1000
    ren.set_shading(2)
    ren.set_empty_space_skipping(True)
    ren.commit()
    shaded = _render(ovr, ren)
    _same_frame(shaded, march, "shading 2 and skipping committed")
    _context_stats(shaded[2], "shading 2 and skipping committed")
    assert ren.slices().range_skipping == 0
    ren.close()


# ---- 2. nothing in front: the same renderer's slice frame, in the product build ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_an_empty_context_gives_the_slice_frame(ovr, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = CC.volume(dtype)
    for how in ("zero alpha table", "scale 0"):
        case = _case(ovr, vol, tf="zero" if how == "zero alpha table" else "dense")
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        for name, cam, clip in (("case", "oblique", None), ("plane+slab", "axis", None), ("plane+slab", "oblique", CLIP), ("plane", "oblique", None)):
            ren.set_camera(ovr.Camera(*PC.CAMERAS[cam], PC.FOVY))
            ren.set_clip_box(*clip) if clip else ren.set_clip_box(None)
            ren.set_slices(CC.SETS[name])
            ren.set_slice_context(OFF)
            ren.commit()
            plain = _render(ovr, ren)
            ren.set_slice_context(FRONT, 1.0 if how == "zero alpha table" else 0.0)
            ren.commit()
            ctx = _render(ovr, ren)
            tag = (np.dtype(dtype).name, am, how, name, cam, clip is not None)
            assert _same(ctx[0], plain[0]) and _same(ctx[1], plain[1]), tag
            box = None
            if clip:
                nz, ny, nx = vol.shape
                box = ovr.clipping.object_box(*clip, *ovr.clipping.volume_constants((nx, ny, nz)))
            steps = _model(ovr, ren, case, CC.SETS[name], scale=1.0 if how == "zero alpha table" else 0.0, clip=box, key=("empty", np.dtype(dtype).name, how, name, cam, clip is not None))[2]["context_steps"]
            assert ctx[2].samples == plain[2].samples + steps and steps > 100 and ctx[2].shaded_samples == 0 and ctx[2].rays == plain[2].rays, (tag, ctx[2].samples, plain[2].samples, steps)
            _context_stats(ctx[2], tag)
            assert (plain[1][..., 2] >= 1).sum() > 50, tag
        ren.close()


# ---- 3. ovr_hip_slice_context_floats against the model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", CC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("am", (0, 1, 2, 3))
def test_context_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
    SC = ovr.slice_context
    eight_bit = np.dtype(dtype).itemsize == 1
    for dims in PC.DIMS:
        vol = CC.volume(dtype, dims)
        org, d, kind = PC.ray_set(dims)
        case = _case(ovr, vol)
        ct, at = PC.tables(case["colors"], case["alphas"])
        tfr = ovr.projection.normalized_range(case["vr"], vol.dtype)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        for rate, scale in ((CC.RATE, 1.0), (1.0, 0.3), (2.5, 1.0)):
            ren.set_volume_sampling_rate(rate)
            ren.set_slice_context(FRONT, scale)
            for name, slices in CC.SETS.items():
                ren.set_slices(slices)
                ren.commit()
                key = ("rays", np.dtype(dtype).name, dims, rate, scale, name)
                if key not in _models:
                    _models[key] = SC.context_rays(vol, org, d, rate, slices, ct, at, tfr, opacity_scale=scale)
                want = _models[key]
                k, v, t, steps, rgba = ren.slice_context_rays(org, d)
                tag = (am, np.dtype(dtype).name, dims, rate, scale, name)
                if EXACT_RUN:
                    assert np.array_equal(k, want["k"]) and np.array_equal(steps, want["steps"]) and _same(t, want["t"]), tag
                    assert _same(rgba, want["rgba"]) and _same(v, want["v"]), (tag, float(np.abs(rgba - want["rgba"]).max()))
                else:
                    # the slice of a ray hangs on the pow's last bit where alpha before it is borderline; its step count wherever ANY loop test was (a long
                    # ray at a high rate nears the threshold in small increments: the dense table flags up to half of this set's rays at rate 2.5, none
                    # under scale 0.3)
                    keep, counted = ~want["borderline_front"], ~want["borderline"]
                    assert counted.sum() > 40 and (scale == 1.0 or counted.all()), tag
                    assert np.array_equal(k[keep], want["k"][keep]) and _same(t[keep], want["t"][keep]) and np.array_equal(steps[counted], want["steps"][counted]), tag
                    assert not np.isnan(rgba).any() and np.abs(rgba - want["rgba"]).max() <= TOL, (tag, float(np.abs(rgba - want["rgba"]).max()))
                    if eight_bit:
                        assert np.abs(v - want["v"])[keep].max() <= TOL, tag
                    else:
                        assert _same(v[keep], want["v"][keep]), tag
                assert (k[kind == "miss"] == 0).all() and not rgba[kind == "miss"].any() and (steps[kind == "miss"] == 0).all(), tag
                if name != "no meet":
                    assert (k > 0).sum() > 10 and (steps > 0).sum() > 30, tag
                else:
                    assert not k.any() and (steps > 0).sum() > 50, tag
        ren.close()


# ---- 4. frames against the model ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = CC.volume(dtype)
    nz, ny, nx = vol.shape
    box = ovr.clipping.object_box(*CLIP, *ovr.clipping.volume_constants((nx, ny, nz)))
    name = np.dtype(dtype).name
    for cam in sorted(PC.CAMERAS):
        case = _case(ovr, vol, cam=cam)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        ren.set_slices(CC.SLICES)
        ren.set_slice_context(FRONT, 1.0)
        ren.commit()
        got = _render(ovr, ren)
        _check_frame(ovr, oracle, case, got, _model(ovr, ren, case, CC.SLICES, key=("frame", name, cam, 1.0, False)), (name, am, cam))
        assert (got[1][..., 2] >= 1).sum() > 50 and got[2].shaded_samples > 500 and ren.slices().range_skipping == 0
        if cam == CC.CAMERA:
            assert set(np.unique(got[1][..., 2]).tolist()) >= {0.0, 1.0, 2.0} and (got[0][..., 3][got[1][..., 2] == 0] >= 0.9999).sum() >= 20   # both slices, and saturated rays
            ren.set_slice_context(FRONT, 0.3)
            ren.set_clip_box(*CLIP)
            ren.commit()
            clipped = _render(ovr, ren)
            _check_frame(ovr, oracle, case, clipped, _model(ovr, ren, case, CC.SLICES, scale=0.3, clip=box, key=("frame", name, cam, 0.3, True)), (name, am, cam, "clip box, scale 0.3"))
            assert not _same(clipped[0], got[0]) and (clipped[1][..., 2] >= 1).sum() > 30
        ren.close()


def test_orthographic_frame_vs_model(ovr, oracle, hip_renderer_factory):
    vol = CC.volume(np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_camera(ovr.Camera((-31.5, 44.25, -39.0), CC.CENTRE, (0.0, 1.0, 0.0), orthographic_height=40.0))
    ren.set_slices(CC.SLICES)
    ren.set_slice_context(FRONT, 1.0)
    ren.commit()
    got = _render(ovr, ren)
    _check_frame(ovr, oracle, case, got, _model(ovr, ren, case, CC.SLICES, camera_kind=ovr.camera.ORTHOGRAPHIC), "orthographic")
    assert (got[1][..., 2] >= 1).sum() > 50
    ren.close()


# ---- 5. samples per pixel, jitter, accumulation --------------------------------------------------------------------------------------------------------------------

def test_accumulation_spp_and_jitter(ovr, oracle, hip_renderer_factory):
    vol = CC.volume(np.float32)
    case = _case(ovr, vol, spp=2)
    noise = np.random.default_rng(77).random((16, 16, 64)).astype(F)
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    hip_setup(ovr, ren, case, accumulate=True)
    ren.set_slices(CC.SLICES)
    ren.set_slice_context(FRONT, 1.0)
    ren.commit()
    one = _render(ovr, ren)
    want1 = _model(ovr, ren, case, CC.SLICES, spp=2, noise=noise, frame_index=1)
    _check_frame(ovr, oracle, case, one, want1, "spp 2, frame 1")
    two = _render(ovr, ren)
    want2 = _model(ovr, ren, case, CC.SLICES, spp=2, noise=noise, frame_index=2)
    assert two[2].frame_index == 2 and not _same(want2[0], want1[0])
    # the accumulated frame: (A1 + A2) / 2 per channel, as write_pixel forms it; the layer is the second frame's
    acc = ((want1[0] + want2[0]).astype(F) / F(2)).astype(F)
    if EXACT_RUN:
        assert _same(two[0], acc) and _same(two[1], want2[1]) and two[2].samples == want2[2]["samples"]
    else:
        compare(oracle, two[0], acc, TOL, name="accumulated")
        keep = ~want2[2]["borderline_front"]
        assert _same(two[1][keep], want2[1][keep]) and abs(int(two[2].samples) - want2[2]["samples"]) <= want2[2]["hinge"] and two[2].rays == want2[2]["rays"]
    ren.close()


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_off_front_off_and_the_accumulation(ovr, hip_renderer_factory):
    vol = CC.volume(np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    ren.set_slices(CC.SLICES)
    ren.commit()
    first = _render(ovr, ren)
    assert ren.slice_context().mode == OFF and ren.slice_context().opacity_scale == 1.0 and ren.slice_context().active == 0 and first[2].frame_index == 1
    assert _render(ovr, ren)[2].frame_index == 2
    ren.set_slice_context(FRONT, 0.5)
    ren.commit()
    front = _render(ovr, ren)
    c = ren.slice_context()
    assert (c.mode, c.opacity_scale, c.active) == (FRONT, 0.5, 1) and front[2].frame_index == 1 and not _same(front[0], first[0]) and front[2].shaded_samples > 0
    assert _render(ovr, ren)[2].frame_index == 2
    ren.set_slice_context(FRONT, 0.5)      # the same values again: still a call - the accumulation starts over
    ren.commit()
    again = _render(ovr, ren)
    _same_frame(again, front, "the same context again")
    assert again[2].frame_index == 1
    ren.set_slice_context(OFF, 0.25)       # the scale is ignored, and stored as 1, in mode OFF
    ren.commit()
    back = _render(ovr, ren)
    _same_frame(back, first, "OFF -> FRONT -> OFF")
    c = ren.slice_context()
    assert (c.mode, c.opacity_scale, c.active) == (OFF, 1.0, 0) and back[2].frame_index == 1 and back[2].shaded_samples == 0 and back[2].pipeline == first[2].pipeline
    # refused values leave the state alone (ValueError where the ABI says EINVAL)
    ren.set_slice_context(FRONT, 0.75)
    ren.commit()
    good = _render(ovr, ren)
    for mode, scale in ((2, 1.0), (-1, 0.5), (FRONT, float("nan")), (FRONT, -0.01), (FRONT, 1.01), (FRONT, INF)):
        with pytest.raises(ValueError, match="ovr_hip_set_slice_context"):
            ren.set_slice_context(mode, scale)
    ren.commit()
    c = ren.slice_context()
    assert (c.mode, c.opacity_scale, c.active) == (FRONT, 0.75, 1)
    kept = _render(ovr, ren)
    assert _same(kept[0], ((good[0] + good[0]).astype(F) / F(2)).astype(F)) and kept[2].frame_index == 2      # no call was recorded: the accumulation goes on
    ren.close()


def test_no_slices_draws_the_march_and_a_twin_gives_the_same_frame(ovr, hip_renderer_factory):
    vol = CC.volume(np.float32)
    case = _case(ovr, vol, shading=2, rate=1.0)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    march = _render(ovr, ren)
    ren.set_slice_context(FRONT, 0.4)
    ren.commit()
    kept = _render(ovr, ren)
    _same_frame(kept, march, "n = 0 with FRONT committed: the march")
    assert ren.slice_context().active == 0 and ren.slice_context().mode == FRONT and march[2].shaded_samples > 0 and march[2].shadow_samples > 0
    ren.set_slices(CC.SLICES)
    ren.set_volume_sampling_rate(CC.RATE)
    ren.commit()
    ctx = _render(ovr, ren)
    assert ren.slice_context().active == 1 and ctx[2].shadow_samples == 0 and not _same(ctx[0], march[0])
    # a fresh renderer given only the final state
    twin = hip_setup(ovr, hip_renderer_factory(), dict(case, rate=CC.RATE))
    twin.set_slices(CC.SLICES)
    twin.set_slice_context(FRONT, 0.4)
    twin.commit()
    _same_frame(_render(ovr, twin), ctx, "a twin with the final state", COUNTERS + ("pipeline", "layout"))
    # errors of the known-answer entry
    import torch
    lib = ovr._lib.load()
    buf = torch.zeros(24, dtype=torch.float32, device=torch.device("cuda", 0))
    twin.set_slice_context(OFF)
    twin.commit()
    assert lib.ovr_hip_slice_context_floats(twin._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1) < 0 and b"no slice context is committed" in lib.ovr_hip_last_error()
    ren.set_slices(None)
    ren.commit()
    assert lib.ovr_hip_slice_context_floats(ren._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1) < 0 and b"no slice is committed" in lib.ovr_hip_last_error()
    twin.close()
    ren.close()


def test_a_device_group_gives_the_single_renderers_frame(ovr, hip_renderer_factory):
    case = _case(ovr, CC.volume(np.float32), size=(56, 40))

    def start(ren):
        hip_setup(ovr, ren, case)
        ren.set_slices(CC.SLICES)
        ren.set_slice_context(FRONT, 0.6)
        ren.commit()
        return ren

    single = start(hip_renderer_factory())
    whole = _render(ovr, single)
    group = ovr.create_renderer("hip", devices=[0, 0])
    try:
        g = _render(ovr, start(group))
        c = group.slice_context()
        assert _same(g[0], whole[0]) and _same(g[1], whole[1]) and (c.mode, c.active) == (FRONT, 1) and abs(c.opacity_scale - 0.6) < 1e-7
        assert (g[2].rays, g[2].samples, g[2].shaded_samples, g[2].active_pixels) == (whole[2].rays, whole[2].samples, whole[2].shaded_samples, whole[2].active_pixels)
        with pytest.raises(ValueError):
            group.set_slice_context(FRONT, 2.0)
    finally:
        group.close()
    assert whole[2].shaded_samples > 500 and (whole[1][..., 2] >= 1).sum() > 100
    single.close()


# ---- 7. the exact-parity build -----------------------------------------------------------------------------------------------------------------------------------------

def test_exact_under_the_exact_parity_build():
    """started the way tests/test_slices_gpu.py starts its child: with the exact-parity build of the kernels the known-answer entry and the frames give the
    model's bits and counters for every voxel type"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
           "context_floats_vs_model or test_frames_vs_model or orthographic_frame_vs_model or accumulation_spp_and_jitter"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 4 * len(CC.DTYPES) + len(MATRIX) + 2 and "failed" not in out.stdout.splitlines()[-1], tail
