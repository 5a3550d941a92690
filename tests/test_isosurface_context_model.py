"""The isosurface-context model (open-volume-renderer_amd/isosurface_context.py, include/ovr_hip.h ovr_hip_set_isosurface_context) on the CPU, pinned from both
sides by frames the project already trusts: with isovalues outside the data range it is the UNMODIFIED oracle's unshaded march bit for bit (its powf mode 2: the
deterministic pair), with an all-zero alpha table or scale 0 it is isosurface.py's translucent (and, with all-ones opacities, opaque) frame bit for bit.  Then the
order of events and samples along a ray, saturation, the scale, a hand-computed ray, and the inputs of the GPU comparison: the rays whose termination rests on the
last bit of the pow are few.  No GPU."""
import os
import re

import numpy as np
import pytest

import isosurface_context_cases as XC
import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ["ovr_hip_set_isosurface_context", "ovr_hip_get_isosurface_context", "ovr_hip_isosurface_context_floats"]
_IDS = lambda d: np.dtype(d).name   # noqa: E731


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _inputs(ovr, oracle, vol, tf="dense", cam=XC.CAMERA):
    w, h = PC.SIZE
    colors, alphas, vr = XC.transfer_function(ovr, tf, vol.dtype)
    ct, at = PC.tables(colors, alphas)
    basis = oracle.camera_basis(*PC.CAMERAS[cam], PC.FOVY, w, h).reshape(4, 3)
    return basis, ct, at, ovr.projection.normalized_range(vr, vol.dtype), (colors, alphas, vr)


def test_entry_points_are_declared_bound_and_exported(ovr):
    hdr = open(os.path.join(ROOT, "include", "ovr_hip.h")).read()
    lib = ovr._lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in ovr._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define OVR_HIP_ISO_CONTEXT_OFF 0\b", hdr) and re.search(r"#define OVR_HIP_ISO_CONTEXT_VOLUME 1\b", hdr)
    assert (ovr._lib.ISO_CONTEXT_OFF, ovr._lib.ISO_CONTEXT_VOLUME) == (ovr.isosurface_context.OFF, ovr.isosurface_context.VOLUME) == (0, 1)
    assert lib.ovr_hip_abi_version() == 11
    assert lib.ovr_hip_set_isosurface_context(None, 0, 1.0) < 0 and lib.ovr_hip_get_isosurface_context(None, None) < 0
    assert lib.ovr_hip_isosurface_context_floats(None, None, None, None, 0, 1) < 0
    for word in ("the context is always unshaded", "the volume casts no shadow on a surface", "ambient occlusion (a", "range and majorant skipping"):
        assert word.lower() in hdr.lower(), word


# ---- identity 1: no crossing on any ray, scale 1: the oracle's unshaded march ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", XC.DTYPES, ids=_IDS)
def test_unreachable_isovalues_give_the_oracles_unshaded_march(ovr, oracle, dtype):
    X = ovr.isosurface_context
    vol = XC.volume(dtype)
    iso = XC.isovalues(XC.UNREACHABLE, dtype)
    for cam, rate in (("axis", 1.0), ("oblique", 2.7)):
        basis, ct, at, tfr, (colors, alphas, vr) = _inputs(ovr, oracle, vol, cam=cam)
        previous = oracle.set_powf_mode(oracle.POWF_DET)
        try:
            ref, grad, cnt = oracle.OracleScene(vol, colors, alphas, vr, PC.CAMERAS[cam], PC.SIZE[0], PC.SIZE[1], fovy=PC.FOVY, rate=rate, shading=0).render()
        finally:
            oracle.set_powf_mode(previous)
        rgba, layer, c = X.frame(vol, basis, PC.SIZE, rate, iso, None, ct, at, tfr)
        assert _same(rgba, ref), (cam, rate, float(np.abs(rgba - ref).max()))
        assert not layer.any() and not grad.any() and c["events"] == 0 and c["shadow_steps"] == 0
        assert c["samples"] == cnt.samples and c["shaded"] == c["lit"] == cnt.shaded_samples and c["rays"] == cnt.rays, (c, cnt.samples, cnt.shaded_samples)
        assert cnt.samples > 3000 and (ref[..., 3] >= 0.9999).sum() >= 10 and ((ref[..., 3] > 0) & (ref[..., 3] < 0.9999)).sum() > 20   # saturated and partial rays alike


# ---- identity 2: an all-zero alpha table, or scale 0: the isosurface frame --------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ("zero alpha table", "scale 0"))
@pytest.mark.parametrize("dtype", XC.DTYPES, ids=_IDS)
def test_an_empty_volume_gives_the_isosurface_frame(ovr, oracle, how, dtype):
    X, ISO = ovr.isosurface_context, ovr.isosurface
    vol = XC.volume(dtype)
    basis, ct, at, tfr, _ = _inputs(ovr, oracle, vol, tf="zero" if how == "zero alpha table" else "dense", cam="oblique")
    scale = 1.0 if how == "zero alpha table" else 0.0
    iso = XC.isovalues(XC.LEVELS, dtype)
    for shading, rate in ((ISO.FULL, XC.RATE), (ISO.GRADIENT, 2.5), (ISO.NONE, 1.0)):
        want = ISO.frame(vol, basis, PC.SIZE, rate, iso, ct, tfr, shading=shading, opacities=XC.SHELLS)
        rgba, layer, c = X.frame(vol, basis, PC.SIZE, rate, iso, XC.SHELLS, ct, at, tfr, opacity_scale=scale, shading=shading)
        tag = (how, np.dtype(dtype).name, shading, rate)
        assert _same(rgba, want[0]) and _same(layer, want[1]), tag
        assert c["samples"] == want[2]["steps"] and c["shaded"] == c["events"] == want[2]["hits"] and c["lit"] == 0 and c["shadow_steps"] == want[2]["shadow_steps"], (tag, c, want[2])
        assert c["events"] > 100 and (layer[..., 2] > 0).sum() > 40 and (shading != ISO.FULL or c["shadow_steps"] > 300), (tag, c)
    # all-ones opacities: the opaque frame (the translucent frame's own identity)
    opaque = ISO.frame(vol, basis, PC.SIZE, XC.RATE, iso, ct, tfr)
    rgba, layer, c = X.frame(vol, basis, PC.SIZE, XC.RATE, iso, None, ct, at, tfr, opacity_scale=scale)
    assert _same(rgba, opaque[0]) and _same(layer, opaque[1]) and c["events"] == opaque[2]["hits"] and c["samples"] == opaque[2]["steps"]


def test_mode_off_is_the_isosurface_frame_and_the_setters_values(ovr):
    X = ovr.isosurface_context
    assert X.commit(X.OFF) == (0, F(1)) and X.commit(X.OFF, 0.25) == (0, F(1)) and X.commit(X.OFF, float("nan")) == (0, F(1))   # ignored, stored as 1
    assert X.commit(X.VOLUME) == (1, F(1)) and X.commit(X.VOLUME, 0.0) == (1, F(0)) and X.commit(X.VOLUME, 0.3) == (1, F(0.3))
    for mode, scale in ((2, 1.0), (-1, 1.0), (X.VOLUME, float("nan")), (X.VOLUME, -0.001), (X.VOLUME, 1.0001), (X.VOLUME, float("inf"))):
        with pytest.raises(ValueError):
            X.commit(mode, scale)
    # active: mode VOLUME, isovalues committed, no slices committed (slices keep their precedence); the mode is kept at n = 0
    assert [X.active(*a) for a in ((X.VOLUME, 2, 0), (X.VOLUME, 0, 0), (X.VOLUME, 2, 1), (X.OFF, 2, 0))] == [1, 0, 0, 0]


# ---- order, saturation, scale ------------------------------------------------------------------------------------------------------------------------------

def _centre_ray(ovr, oracle, vol, levels, opacities, tf="dense", scale=1.0, rate=1.0, shading=0):
    """one ray along +x through the middle of the `ball` volume (its longest axis: the ray enters and leaves through the exterior)"""
    X = ovr.isosurface_context
    colors, alphas, vr = XC.transfer_function(ovr, tf, vol.dtype)
    ct, at = PC.tables(colors, alphas)
    tfr = ovr.projection.normalized_range(vr, vol.dtype)
    org, d = np.array([[-5.0, 16.5, 9.0]], F), np.array([[1.0, 0.0, 0.0]], F)
    return X.context_rays(vol, org, d, rate, XC.isovalues(levels, vol.dtype), opacities, ct, at, tfr, opacity_scale=scale, shading=shading)


def test_nested_shells_interleave_with_the_volume_in_tm_order(ovr, oracle):
    vol = XC.volume(np.float32)
    r = _centre_ray(ovr, oracle, vol, XC.LEVELS, (0.05, 0.05), scale=0.02)   # thin enough for the ray to leave the box unsaturated
    assert [e["k"] for e in r["events"][0]] == [0, 1, 1, 0] and r["A"][0] < XC.ERT
    order = r["order"][0]
    # a surface in front of its step's own sample: ("event", i, k) precedes ("sample", i), and the steps never go back
    steps = [item[1] for item in order]
    assert steps == sorted(steps)
    for n, item in enumerate(order):
        if item[0] == "event":
            assert ("sample", item[1]) in order[n + 1:] and ("sample", item[1]) not in order[:n], item
    kinds = "".join("E" if item[0] == "event" else "s" for item in order)
    assert re.fullmatch(r"s+E(s+)E(s+)E(s+)Es+", kinds), kinds        # volume samples in front of, between and behind the four events
    t = [e["t"] for e in r["events"][0]]
    assert t == sorted(t) and len(set(t)) == 4
    assert r["steps"][0] == 40 and r["lit"][0] == sum(1 for item in order if item[0] == "sample") and r["n_events"][0] == 4


def test_saturation_by_the_volume_in_front_of_a_shell_gives_no_event(ovr):
    """seven voxels of 0.95 in front of one of 0.1 under the alpha table (0, 1): the ray saturates after four steps (0.05^4 < 1e-4), three steps in front of the
    falling crossing of 0.5 - no event, a zero layer; thinned to a twentieth it reaches the shell"""
    X = ovr.isosurface_context
    vol = np.array([[[0.95] * 7 + [0.1]]], F)
    ct, at = np.array([[0, 0, 1], [1, 0, 0]], F), np.array([0, 1], F)
    org, d = np.array([[-1.0, 0.5, 0.5]], F), np.array([[1.0, 0.0, 0.0]], F)
    r = X.context_rays(vol, org, d, 1.0, [0.5], [1.0], ct, at, (F(0), F(1)), shading=0)
    thin = X.context_rays(vol, org, d, 1.0, [0.5], [1.0], ct, at, (F(0), F(1)), opacity_scale=0.05, shading=0)
    assert r["n_events"][0] == 0 and r["A"][0] >= XC.ERT and r["iso"][0] == 0 and r["t"][0] == 0 and not r["events"][0] and r["steps"][0] == 4 and r["lit"][0] == 4
    assert thin["n_events"][0] == 1 and thin["rgba"][0, 3] == 1 and thin["steps"][0] == 8 and thin["iso"][0] == F(0.5) and thin["events"][0][0]["i"] == 7
    # the saturated ray on the `ball`: the far halves of the nested shells lie behind the dense core and are not met
    far = _centre_ray(ovr, None, XC.volume(np.float32), XC.LEVELS, XC.SHELLS)
    assert [e["k"] for e in far["events"][0]] == [0, 1] and far["A"][0] >= XC.ERT


def test_saturation_by_an_event_leaves_the_steps_sample_out(ovr, oracle):
    vol = XC.volume(np.float32)
    r = _centre_ray(ovr, oracle, vol, XC.LEVELS, (1.0, 1.0))
    ev = r["events"][0]
    assert len(ev) == 1 and r["A"][0] == 1 and ("sample", ev[0]["i"]) not in r["order"][0] and r["order"][0][-1] == ("event", ev[0]["i"], 0)
    assert r["steps"][0] == ev[0]["i"] + 1 and r["lit"][0] == sum(1 for item in r["order"][0] if item[0] == "sample")
    # the same ray with a translucent first shell takes that step's sample behind the event
    r2 = _centre_ray(ovr, oracle, vol, XC.LEVELS, (0.5, 1.0))
    assert ("sample", ev[0]["i"]) in r2["order"][0] and r2["lit"][0] > r["lit"][0]


def test_the_scale_thins_the_volume_and_leaves_the_shells_alone(ovr, oracle):
    vol = XC.volume(np.float32)
    full = _centre_ray(ovr, oracle, vol, XC.LEVELS, XC.SHELLS)
    thin = _centre_ray(ovr, oracle, vol, XC.LEVELS, XC.SHELLS, scale=0.3)
    none = _centre_ray(ovr, oracle, vol, XC.LEVELS, XC.SHELLS, scale=0.0)
    # the first event: A grows by tr * alpha_k with alpha_k untouched; in front of it the volume's opacity shrinks with the scale
    a_front = [F(F(r["events"][0][0]["A"] - F(XC.SHELLS[0])) / F(1 - XC.SHELLS[0])) for r in (full, thin, none)]
    assert a_front[0] > a_front[1] > a_front[2] == 0 and none["events"][0][0]["A"] == F(XC.SHELLS[0])
    assert _same([e["t"] for e in full["events"][0][:2]], [e["t"] for e in none["events"][0][:2]])      # the crossings themselves do not move
    assert none["lit"][0] == 0 and thin["lit"][0] >= full["lit"][0] > 0


# ---- the frame ------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_hand_computed_three_step_ray(ovr):
    """a 3 x 1 x 1 volume (0.2, 0.6, 0.2), a ray along x through the voxel centres at rate 1: steps at tm = 0.5, 1.5, 2.5 with s = the voxels; isovalue 0.4 with
    opacity 0.5 is crossed rising at step 1 and falling at step 2.  Two-entry tables: colour (v, 0, 1 - v), alpha v.  Unshaded, so the events' colour is the
    table's at 0.4.  Every operation below is written out, in the definition's order"""
    X = ovr.isosurface_context
    vol = np.array([[[0.2, 0.6, 0.2]]], F)
    ct, at = np.array([[0, 0, 1], [1, 0, 0]], F), np.array([0, 1], F)
    r = X.context_rays(vol, np.array([[-1.0, 0.5, 0.5]], F), np.array([[1.0, 0.0, 0.0]], F), 1.0, [0.4], [0.5], ct, at, (F(0), F(1)), shading=0)
    fma = ovr.lighting.fma
    A, C = F(0), np.zeros(3, F)

    def sample(s, A, C):       # dt = 1: the opacity correction keeps a_tf
        rgb, a = np.array([s, 0, F(1) - s], F), F(s)
        tr = F(F(1) - A)
        return fma(tr, a, A), fma((tr * rgb).astype(F), a, C)

    def event(A, C):
        rgb, a = np.array([F(0.4), 0, F(1) - F(0.4)], F), F(0.5)
        tr = F(F(1) - A)
        return fma(tr, a, A), fma((tr * rgb).astype(F), a, C)

    A, C = sample(F(0.2), A, C)
    A, C = event(A, C)
    A, C = sample(F(0.6), A, C)
    A, C = event(A, C)
    A, C = sample(F(0.2), A, C)
    assert r["steps"][0] == 3 and r["n_events"][0] == 2 and r["lit"][0] == 3 and r["order"][0] == [("sample", 0), ("event", 1, 0), ("sample", 1), ("event", 2, 0), ("sample", 2)]
    assert _same(r["A"][0], A) and _same(r["rgba"][0, :3], (C / A).astype(F)) and _same(r["rgba"][0, 3], A), (r["rgba"], A, C)
    assert r["iso"][0] == F(0.4) and abs(float(r["t"][0]) - 2.0) < 1e-5        # the rising crossing lies halfway between the voxel centres 0.5 and 1.5: x = 1, t = 2


def test_frames_with_spp_clip_box_orthographic_camera_and_vertex_centred_grid(ovr, oracle):
    X, ISO = ovr.isosurface_context, ovr.isosurface
    vol = XC.volume(np.float32)
    basis, ct, at, tfr, _ = _inputs(ovr, oracle, vol)
    zero = np.zeros_like(at)
    iso = XC.isovalues(XC.LEVELS, np.float32)
    nz, ny, nx = vol.shape
    box = ovr.clipping.object_box(*XC.CLIP, *ovr.clipping.volume_constants((nx, ny, nz)))
    noise = np.random.default_rng(7).random((16, 16, 64)).astype(F)
    ortho = tuple(np.asarray(v, F) for v in ovr.camera.basis((-31.5, 44.25, -39.0), (20.0, 16.5, 9.0), (0.0, 1.0, 0.0), *PC.SIZE, orthographic_height=40.0))
    variants = [dict(spp=2, noise=noise, frame_index=3), dict(clip=box), dict(vertex_centred=True), dict(camera_kind=ovr.camera.ORTHOGRAPHIC)]
    plain = X.frame(vol, basis, PC.SIZE, XC.RATE, iso, XC.SHELLS, ct, at, tfr)
    for kw in variants:
        b = ortho if "camera_kind" in kw else basis
        got = X.frame(vol, b, PC.SIZE, XC.RATE, iso, XC.SHELLS, ct, at, tfr, **kw)
        empty = X.frame(vol, b, PC.SIZE, XC.RATE, iso, XC.SHELLS, ct, zero, tfr, **kw)
        want = ISO.frame(vol, b, PC.SIZE, XC.RATE, iso, ct, tfr, opacities=XC.SHELLS, **kw)
        tag = sorted(kw)
        assert _same(empty[0], want[0]) and _same(empty[1], want[1]) and empty[2]["events"] == want[2]["hits"] and empty[2]["samples"] == want[2]["steps"], tag
        assert got[2]["lit"] > 300 and got[2]["events"] > 50 and not _same(got[0], plain[0]) and not _same(got[0], empty[0]), (tag, got[2]["lit"], got[2]["events"])
        assert (got[0][..., 3] >= empty[0][..., 3]).all() and got[2]["rays"] == PC.SIZE[0] * PC.SIZE[1] * kw.get("spp", 1), tag


# ---- the borderline cap ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", XC.DTYPES, ids=_IDS)
def test_borderline_rays_of_the_committed_case_are_at_most_one_percent(ovr, oracle, dtype):
    X = ovr.isosurface_context
    vol = XC.volume(dtype)
    basis, ct, at, tfr, _ = _inputs(ovr, oracle, vol)
    for scale in XC.SCALES:
        rgba, layer, c = X.frame(vol, basis, PC.SIZE, XC.RATE, XC.isovalues(XC.LEVELS, dtype), XC.SHELLS, ct, at, tfr, opacity_scale=scale)
        with_event = int((layer[..., 2] > 0).sum())
        print(np.dtype(dtype).name, scale, "rays with an event", with_event, "borderline", int(c["borderline"].sum()), "of them with a crossing", int(c["borderline_event"].sum()))
        assert with_event >= 60 and c["borderline_event"].sum() <= XC.BORDER_CAP * with_event, (scale, with_event, int(c["borderline_event"].sum()))
        assert c["events"] > 150 and c["lit"] > 500 and c["shadow_steps"] > 300
        assert scale != 1.0 or (rgba[..., 3] >= XC.ERT).sum() >= 20          # the dense volume saturates rays at scale 1
