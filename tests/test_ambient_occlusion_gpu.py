"""Ambient occlusion of the isosurface frames on the GPU (include/ovr_hip.h ovr_hip_set_ambient_occlusion) against the numpy model
open-volume-renderer_amd/isosurface.py, fed with the HOST's direction table.  "Bits" are float32 bit patterns.  O, the events, k, t*, A, the shadow term, the
layer, the steps and the counters are the model's bits in the product build too (for u8 through isosurface.product_sampler).  Normals and colours use the
product's reciprocal multiply and v_rsq_f32: helpers.compare's float bar there (atol 2e-4 on normals), bits under the exact-parity library
(test_ao_is_exact_under_the_exact_parity_build).  The rotation of the direction table follows the frame index the statistics report: the model is asked for
that frame."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ambient_occlusion_cases as AC
import isosurface_cases as IC
import projection_cases as PC
from helpers import EXACT_RUN, compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
RENDERBATCH = os.path.join(ROOT, "oracle", "_ref", "renderbatch")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
F = np.float32
INF = float("inf")
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
TOL = 2e-4   # helpers.compare's float bar
LIGHT = (0.3, 0.8, -0.52)
MIXED = (0.3, 0.4, 0.5, 1.0)
MAX_EVENTS = 8
SIZE = (32, 24)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, cam="oblique", rate=1.0, shading=2, spp=1, size=SIZE):
    colors, alphas, vr = PC.transfer_function(ovr, "sparse", vol.dtype)
    fovy = IC.FOVY if isinstance(cam, str) else AC.FOVY
    cam = IC.CAMERAS[cam] if isinstance(cam, str) else cam
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=cam, size=size, shading=shading, rate=rate, spp=spp, convention=0, spacing=(1.0, 1.0, 1.0),
                origin=(0.0, 0.0, 0.0), fovy=fovy)


def _start(ovr, ren, case, iso, opacities, ao=None, skipping=False, accumulate=False):
    hip_setup(ovr, ren, case, accumulate=accumulate)
    ren.set_light_direction(LIGHT, 1.0)
    ren.set_isosurfaces(iso, opacities)
    ren.set_empty_space_skipping(skipping)
    if ao is not None:
        ren.set_ambient_occlusion(*ao)
    ren.commit()
    return ren


def _render(ovr, ren):
    ren.render()
    rgba, layer = hip_frame(ovr, ren)
    return rgba, layer, ren.stats()


def _sampler(ovr, vol):
    return None if EXACT_RUN else ovr.isosurface.product_sampler(vol)


def _model(ovr, oracle, case, iso, opacities, ren, **kw):
    """the model's frame of a case with the renderer's committed AO state and the HOST's table"""
    I, P = ovr.isosurface, ovr.projection
    w, h = case["size"]
    basis = kw.pop("basis", None)
    if basis is None:
        basis = oracle.camera_basis(*case["cam"], case["fovy"], w, h).reshape(4, 3)
    ct, _ = PC.tables(case["colors"], case["alphas"])
    s = ren.get_ambient_occlusion()
    ao = (ren.ambient_occlusion_directions(), s.distance) if s.samples else None
    kw.setdefault("frame_index", ren.stats().frame_index)       # the frame rendered last
    return I.frame(case["vol"], basis, case["size"], case["rate"], iso, ct, P.normalized_range(case["vr"], case["vol"].dtype), shading=case["shading"],
                   sampler=_sampler(ovr, case["vol"]), opacities=opacities, light=LIGHT, ao=ao, **kw)


def _check_frame(oracle, case, got, want, name, skipping=False):
    rgba, layer, st = got
    ref, ref_layer, cnt = want
    assert _same(layer, ref_layer), (name, float(np.abs(layer - ref_layer).max()))
    assert _same(rgba[..., 3], ref[..., 3]), (name, "A", float(np.abs(rgba[..., 3] - ref[..., 3]).max()))
    if EXACT_RUN:
        assert _same(rgba, ref), (name, float(np.abs(rgba - ref).max()))
    else:
        compare(oracle, rgba, ref, name=str(name))
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"] and st.samples + st.skipped_samples == cnt["steps"] and st.shaded_samples == cnt["hits"], \
        (name, st.samples + st.skipped_samples, cnt["steps"], st.shaded_samples, cnt["hits"])
    assert st.shadow_samples + st.skipped_shadow_samples == cnt["shadow_steps"] + cnt["ao_steps"], (name, st.shadow_samples + st.skipped_shadow_samples, cnt["shadow_steps"], cnt["ao_steps"])
    if not skipping:
        assert st.skipped_samples == 0 and st.skipped_shadow_samples == 0 and st.shadow_samples == cnt["shadow_fetched"] + cnt["ao_fetched"], name
    assert st.layout == 0 and st.pipeline == 1 and st.tuning == 0, name


# ---- 1. the direction table and ovr_hip_isosurface_ao_floats against the model --------------------------------------------------------------------

def test_the_hosts_table_is_the_models_to_one_ulp(ovr, hip_renderer_factory):
    ren = hip_setup(ovr, hip_renderer_factory(), _case(ovr, AC.ramp()))
    assert ren.ambient_occlusion_directions().shape == (16, 0, 3)
    for K in range(1, 17):
        ren.set_ambient_occlusion(K, 3.0)
        ren.commit()
        host, model = ren.ambient_occlusion_directions(), ovr.isosurface.ao_directions(K)
        assert host.shape == model.shape == (16, K, 3)
        near = (host == model) | (np.abs(_bits(np.abs(host)).astype(np.int64) - _bits(np.abs(model)).astype(np.int64)) <= 1) & (np.sign(host) == np.sign(model))
        assert near.all(), K
    ren.close()


@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("K", AC.KS)
def test_ao_floats_vs_model(ovr, hip_renderer_factory, K, dtype):
    """all sixteen rotations over a seeded ray set, R in {3, inf}, both walks: bits for O, the events, t*, A, the shadow term and the step counts"""
    I = ovr.isosurface
    dims = IC.DIMS[0]
    vol = IC.volume("ball", dtype, dims)
    org, d, kind = PC.ray_set(dims)
    rot = np.arange(len(org)) & 15
    iso = IC.scaled(IC.NESTED["ball"], dtype)
    ren = _start(ovr, hip_renderer_factory(), _case(ovr, vol), iso[::-1], MIXED[::-1], ao=(K, 3.0))
    occluded = events = 0
    for R in (3.0, INF):
        ren.set_ambient_occlusion(K, R)
        ren.commit()
        s = ren.get_ambient_occlusion()
        assert (s.samples, s.distance, s.rotations, s.active) == (K, R, 16, 1)
        table = ren.ambient_occlusion_directions()
        for skip in (False, True):
            want = I.trace_rays(vol, org, d, 1.0, iso, light=LIGHT, sampler=_sampler(ovr, vol), opacities=MIXED, skipping=skip, ao=(table, R, rot))
            f = want["flat"]
            first = np.concatenate([[0], np.cumsum(want["n_events"])[:-1]])
            slot = np.arange(len(f["ray"])) - first[f["ray"]]
            for m in range(16):
                rays = np.flatnonzero(rot == m)
                got = ren.isosurface_ao_rays(org[rays], d[rays], m, MAX_EVENTS, skip)
                name = (K, R, skip, m)
                assert np.array_equal(got["events"], want["n_events"][rays]) and _same(got["A"], want["A"][rays]), name
                assert np.array_equal(got["steps"], want["steps"][rays]) and np.array_equal(got["shadow_steps"], want["shadow_steps"][rays]), name
                keep = np.isin(f["ray"], rays) & (slot < MAX_EVENTS)
                r, e = np.searchsorted(rays, f["ray"][keep]), slot[keep]
                assert np.array_equal(got["k"][r, e], f["k"][keep]), name
                for key, mine in (("t", "t"), ("shadow", "shadow"), ("A_after", "A")):
                    assert _same(got[key][r, e], f[mine][keep]), (name, key)
                if EXACT_RUN:
                    assert _same(got["normal"][r, e], f["normal"][keep]), name
                else:
                    assert np.allclose(got["normal"][r, e], f["normal"][keep], rtol=0, atol=TOL, equal_nan=True), name
                full = want["n_events"][rays] <= MAX_EVENTS       # (the ray's totals cover every event, the record the first MAX_EVENTS)
                assert _same(got["O"][r, e], f["O"][keep]), (name, "O", float(np.abs(got["O"][r, e] - f["O"][keep]).max()))
                assert np.array_equal(got["ao_steps"][full], want["ao_steps"][rays][full]) and np.array_equal(got["ao_fetched"][full], want["ao_fetched"][rays][full]), name
                empty = np.ones(got["O"].shape, bool)
                empty[r, e] = False
                assert not got["O"][empty].any() and not got["t"][empty].any(), (name, "the rest is zeros")
            if not skip:
                occluded += int(((f["O"] > 0) & (f["O"] < 1)).sum())
                events += len(f["O"])
    ren.close()
    assert events > 100 and occluded > 30, (events, occluded)


def test_ao_is_exact_under_the_exact_parity_build():
    """started the way test_layers_are_exact_under_the_exact_parity_build starts its child: with the exact-parity build of the kernels normals, shade factors and
    colours give the model's bits too"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(ao_floats_vs_model and 5) or frames_vs_model"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 3 + 4 and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 2. frames against the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opacities", (None, MIXED), ids=("opaque", "translucent"))
@pytest.mark.parametrize("shading", (1, 2), ids=("gradient", "full"))
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, shading, opacities):
    if opacities is None:       # the lumpy outer level sets of the synthetic volume (a convex ball, seen from outside, occludes nothing)
        vol, iso = ovr.synth.make_volume(32, np.float32), np.array([0.2, 0.35], F)
        case = _case(ovr, vol, cam=ovr.synth.make_camera("oblique", 32)[:3], shading=shading)
    else:                       # nested translucent shells
        vol = IC.volume("ball", np.float32)
        iso = IC.scaled(IC.NESTED["ball"], np.float32)
        case = _case(ovr, vol, shading=shading)
    ren = _start(ovr, hip_renderer_factory(), case, iso, opacities, ao=(5, 6.0))
    got = _render(ovr, ren)
    want = _model(ovr, oracle, case, iso, opacities, ren)
    _check_frame(oracle, case, got, want, (shading, opacities))
    assert want[2]["ao_steps"] > want[2]["hits"] > 100 and ren.get_ambient_occlusion().active == 1
    off = _start(ovr, hip_renderer_factory(), case, iso, opacities)
    plain = _render(ovr, off)
    assert _same(plain[1], got[1]) and (got[0][..., :3] <= plain[0][..., :3]).all() and (got[0][..., :3] < plain[0][..., :3]).any(-1).sum() > 30, "the occlusion darkens, and nothing else"
    assert plain[2].shadow_samples == want[2]["shadow_fetched"] and off.get_ambient_occlusion().active == 0
    ren.close()
    off.close()


# ---- 3. identities -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shading", (1, 2))
def test_a_plane_and_a_short_radius_give_the_frame_without_ao(ovr, hip_renderer_factory, shading):
    """while the AO kernels run: in front of a plane nothing occludes; inside the cavity nothing occludes within R = 2; K = 0 through the setter is the parent's frame"""
    for vol, cam, iso, ao in ((AC.ramp(), AC.RAMP_CAMERA, [0.5], (5, INF)), (AC.ramp(), AC.RAMP_CAMERA, [0.5], (16, INF)), (AC.cavity(), AC.CAVITY_CAMERA, [AC.level(AC.CAVITY_RADIUS)], (5, 2.0))):
        case = _case(ovr, vol, cam=cam, shading=shading)
        never = _start(ovr, hip_renderer_factory(), case, iso, None)
        on = _start(ovr, hip_renderer_factory(), case, iso, None, ao=ao)
        a, b = _render(ovr, never), _render(ovr, on)
        assert on.get_ambient_occlusion().active == 1 and a[2].shaded_samples > 100
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and [getattr(a[2], k) for k in COUNTERS if "shadow" not in k] == [getattr(b[2], k) for k in COUNTERS if "shadow" not in k]
        assert b[2].shadow_samples > a[2].shadow_samples, "the AO walks walked"
        on.set_ambient_occlusion(0, -5.0)       # (the distance is not read while K == 0)
        on.commit()
        c = _render(ovr, on)
        s = on.get_ambient_occlusion()
        assert (s.samples, s.distance, s.active) == (0, INF, 0)
        assert _same(a[0], c[0]) and _same(a[1], c[1]) and [getattr(a[2], k) for k in COUNTERS] == [getattr(c[2], k) for k in COUNTERS]
        never.close()
        on.close()


def test_the_cavity_is_black_under_an_ambient_material(ovr, hip_renderer_factory):
    """O = 1.0f at every hit: with kd = ks = 0 the hits' rgb is 0 and a = 1"""
    case = _case(ovr, AC.cavity(), cam=AC.CAVITY_CAMERA)
    for K in AC.KS:
        ren = hip_renderer_factory()
        ren.set_material(0.5, 0.0, 0.0, 0.0)
        _start(ovr, ren, case, [AC.level(AC.CAVITY_RADIUS)], None, ao=(K, INF))
        rgba, layer, st = _render(ovr, ren)
        assert st.shaded_samples == SIZE[0] * SIZE[1] and (rgba[..., 3] == 1).all() and not rgba[..., :3].any() and (layer[..., 2] == 1).all()
        ren.close()


@pytest.mark.parametrize("shading", (0, 2))
def test_frames_without_an_ambient_term_on_a_surface_never_change(ovr, hip_renderer_factory, shading):
    """a march frame, a MAXIMUM frame and an isosurface frame under NONE with K = 8 committed: bit for bit what they are without it, counters equal"""
    vol = PC.volume("smooth", np.float32)
    case = _case(ovr, vol, shading=shading)
    never, kept = hip_setup(ovr, hip_renderer_factory(), case), hip_setup(ovr, hip_renderer_factory(), case)
    kept.set_ambient_occlusion(8, 4.0)
    kept.commit()
    steps = []
    for step in ("march", "maximum", "isosurfaces under NONE"):
        for ren in (never, kept):
            if step == "maximum":
                ren.set_projection(1)
            if step == "isosurfaces under NONE":
                ren.set_shading(0)
                ren.set_isosurfaces(IC.NESTED["smooth"], MIXED)
            ren.commit()
        a, b = _render(ovr, never), _render(ovr, kept)
        s = kept.get_ambient_occlusion()
        assert (s.samples, s.distance, s.active) == (8, 4.0, 0), step
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and [getattr(a[2], k) for k in COUNTERS] == [getattr(b[2], k) for k in COUNTERS], step
        assert a[2].samples > 0
        steps.append(a[0])
    assert not _same(steps[0], steps[1]) and not _same(steps[1], steps[2])
    never.close()
    kept.close()


# ---- 4. invariants -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (np.float32, np.uint8), ids=lambda d: np.dtype(d).name)
def test_range_skipping_is_invisible(ovr, hip_renderer_factory, dtype):
    vol = IC.volume("ball", dtype)
    iso = IC.scaled(IC.NESTED["ball"], dtype)
    case = _case(ovr, vol, rate=2.5)
    plain, skipping = (_start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(4, 7.0), skipping=s) for s in (False, True))
    a, b = _render(ovr, plain), _render(ovr, skipping)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert a[2].skipped_samples == 0 and a[2].samples == b[2].samples + b[2].skipped_samples and a[2].rays == b[2].rays and a[2].shaded_samples == b[2].shaded_samples
    assert a[2].skipped_shadow_samples == 0 and a[2].shadow_samples == b[2].shadow_samples + b[2].skipped_shadow_samples and b[2].skipped_shadow_samples > 0
    assert skipping.get_isosurface_layers().range_skipping == 1 and b[2].skipping_kernels == 1
    plain.close()
    skipping.close()


def test_range_skipping_behind_update_volume(ovr, hip_renderer_factory):
    vol = IC.volume("slab", np.float32)
    patch = np.full((3, 9, 11), 0.97, F)     # inside the dim cells behind the slab (z >= 15), whose ranges excluded the isovalues
    lower = (14, 12, 15)
    patched = vol.copy()
    patched[lower[2]:lower[2] + 3, lower[1]:lower[1] + 9, lower[0]:lower[0] + 11] = patch
    case = _case(ovr, vol, cam=IC.BEHIND, rate=2.5)
    iso, op = [0.5, 0.8], (0.4, 0.6)
    ren = _start(ovr, hip_renderer_factory(), case, iso, op, ao=(4, INF), skipping=True)
    before = _render(ovr, ren)
    ren.update_volume(patch, lower)
    after = _render(ovr, ren)
    plain_ren = _start(ovr, hip_renderer_factory(), dict(case, vol=patched), iso, op, ao=(4, INF), skipping=False)
    plain = [_render(ovr, plain_ren) for _ in range(2)][1]       # (its second frame, like `after`: the same rotations)
    assert after[2].frame_index == plain[2].frame_index == 2 and _same(after[0], plain[0]) and _same(after[1], plain[1]) and not _same(after[0], before[0])
    assert after[2].shadow_samples + after[2].skipped_shadow_samples == plain[2].shadow_samples and after[2].shaded_samples == plain[2].shaded_samples
    ren.close()
    plain_ren.close()


def _noise():
    return np.random.default_rng(77).random((16, 16, 64)).astype(F)


def test_accumulation_takes_every_rotation(ovr, oracle, hip_renderer_factory):
    """sixteen accumulated frames against the mean of the model's sixteen frames (each pixel sees all sixteen rotations); two samples per pixel under the
    blue-noise jitter against the model's frame"""
    vol = IC.volume("ball", np.float32)
    iso = IC.scaled(IC.NESTED["ball"][:2], np.float32)
    case = _case(ovr, vol, shading=1, size=(24, 18))
    ren = _start(ovr, hip_renderer_factory(), case, iso, (0.5, 1.0), ao=(2, 8.0), accumulate=True)
    total = np.zeros((18, 24, 4), F)
    frames = []
    for n in range(1, 17):
        got = _render(ovr, ren)
        want = _model(ovr, oracle, case, iso, (0.5, 1.0), ren, frame_index=n)
        total = (total + want[0]).astype(F)
        frames.append(want[0])
        assert got[2].frame_index == n and (n > 1 or _same(got[1], want[1]))
        compare(oracle, got[0], (total / F(n)).astype(F), name="accumulated %d" % n)
    assert len({f.tobytes() for f in frames}) >= 4, "the rotation did not advance with the frame"
    ren.set_ambient_occlusion(2, 8.0)             # every call resets the accumulation
    ren.commit()
    assert _render(ovr, ren)[2].frame_index == 1
    ren.close()
    case2 = _case(ovr, vol, shading=2, spp=2, size=(24, 18))
    noise = _noise()
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    _start(ovr, ren, case2, iso, (0.5, 1.0), ao=(3, INF))
    got = _render(ovr, ren)
    _check_frame(oracle, case2, got, _model(ovr, oracle, case2, iso, (0.5, 1.0), ren, spp=2, noise=noise, frame_index=1), "spp 2")
    ren.close()


def test_sparse_sampling_and_reconstruction(ovr, hip_renderer_factory):
    case = _case(ovr, IC.volume("ball", np.float32), size=(48, 36))
    ren = hip_renderer_factory()
    ren.set_noise_tile(_noise())
    _start(ovr, ren, case, IC.NESTED["ball"], MIXED, ao=(3, 6.0))
    other = _start(ovr, hip_renderer_factory(), case, IC.NESTED["ball"], MIXED, ao=(3, 6.0))
    frames = [_render(ovr, other) for _ in range(3)]      # the dense frames 1, 2, 3: a pixel's rotation follows the frame index
    other.close()
    dense = _render(ovr, ren)
    assert _same(dense[0], frames[0][0])
    ren.set_sparse_sampling(True)
    ren.set_focus((0.5, 0.5), 0.3, 0.2)
    ren.commit()
    sparse = _render(ovr, ren)
    xy = ren.sparse_mask(sparse[2].frame_index).reshape(-1, 2)
    mask = np.zeros(dense[0].shape[:2], bool)
    mask[xy[:, 1], xy[:, 0]] = True
    assert 50 < mask.sum() < mask.size - 50 and sparse[2].active_pixels == mask.sum()
    dense = frames[sparse[2].frame_index - 1]
    assert _same(sparse[0][mask], dense[0][mask]) and _same(sparse[1][mask], dense[1][mask])      # the rotation is the pixel's, list or no list
    assert not sparse[0][~mask].any() and not sparse[1][~mask].any()
    ren.set_reconstruction(1)
    ren.commit()
    filled = _render(ovr, ren)
    xy = ren.sparse_mask(filled[2].frame_index).reshape(-1, 2)
    mask[:] = False
    mask[xy[:, 1], xy[:, 0]] = True
    dense = frames[filled[2].frame_index - 1]
    assert _same(filled[0][mask], dense[0][mask]) and _same(filled[1][mask], dense[1][mask]) and filled[0][~mask].any()
    ren.close()


def test_clip_box_cuts_the_occluders_away(ovr, oracle, hip_renderer_factory):
    """AO rays are clipped: under a clip box the frame is the model's, and a box that keeps the near wall of the cavity's far side alone leaves nothing to occlude"""
    vol = IC.volume("ball", np.float32)
    nz, ny, nx = vol.shape
    case = _case(ovr, vol, rate=2.5)
    iso = IC.scaled(IC.NESTED["ball"], np.float32)
    lower, upper = (5.5, -INF, 3.0), (19.0, 20.25, INF)
    inv, wp = ovr.clipping.volume_constants((nx, ny, nz))
    box = ovr.clipping.object_box(lower, upper, inv, wp)
    for skip in (False, True):
        ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(4, INF), skipping=skip)
        unclipped = _render(ovr, ren)
        ren.set_clip_box(lower, upper)
        ren.commit()
        got = _render(ovr, ren)
        _check_frame(oracle, case, got, _model(ovr, oracle, case, iso, MIXED, ren, clip=box, skipping=skip), ("clip", skip), skipping=skip)
        assert not _same(got[0], unclipped[0])
        ren.close()
    # the cavity seen from its centre under an ambient-only material: whole, every walk ends on the far wall and the frame is black; with all but a cap of the
    # wall cut away most walks run into the cut and find nothing - no pixel gets darker, the cap is lit, and the frame is the model's
    ccase = _case(ovr, AC.cavity(), cam=((16.0, 16.0, 16.0), (30.0, 16.0, 16.0), (0.0, 1.0, 0.0)), shading=1)
    level = [AC.level(AC.CAVITY_RADIUS)]
    on = hip_renderer_factory()
    on.set_material(0.5, 0.0, 0.0, 0.0)
    _start(ovr, on, ccase, level, None, ao=(5, INF))
    full = _render(ovr, on)
    cut = ((25.0, -INF, -INF), (INF, INF, INF))
    on.set_clip_box(*cut)
    on.commit()
    a = _render(ovr, on)
    cbox = ovr.clipping.object_box(cut[0], cut[1], *ovr.clipping.volume_constants((AC.CAVITY_N,) * 3))
    _check_frame(oracle, ccase, a, _model(ovr, oracle, ccase, level, None, on, clip=cbox, material=(0.5, 0.0, 0.0, 0.0)), "the cap")
    hit = a[0][..., 3] == 1
    assert not full[0][..., :3].any() and hit.sum() > 100 and (a[0][hit][:, :3].max(1) > 0).sum() > hit.sum() // 2
    on.close()


def test_orthographic_camera(ovr, oracle, hip_renderer_factory):
    K, I, P = ovr.camera, ovr.isosurface, ovr.projection
    vol = IC.volume("ball", np.float32)
    iso = IC.scaled(IC.NESTED["ball"], np.float32)
    for shading, skip in ((2, False), (1, True)):
        case = _case(ovr, vol, shading=shading)
        ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(4, 9.0), skipping=skip)
        ren.set_camera(ovr.Camera(*IC.CAMERAS["oblique"], orthographic_height=30.0))
        ren.commit()
        c = ren.get_camera()
        basis = tuple(np.array(list(v), F) for v in (c.pos, c.dir, c.hor, c.ver))
        got = _render(ovr, ren)
        want = _model(ovr, oracle, case, iso, MIXED, ren, basis=basis, skipping=skip, camera_kind=K.ORTHOGRAPHIC)
        _check_frame(oracle, case, got, want, ("orthographic", shading, skip), skipping=skip)
        assert want[2]["hits"] > 100 and want[2]["ao_steps"] > 0
        ren.close()


def test_image_shards_and_device_group(ovr, hip_renderer_factory):
    size, tw, th = (48, 36), 16, 8
    case = _case(ovr, IC.volume("ball", np.float32), size=size)
    iso = IC.NESTED["ball"]
    total = lambda s: (s.rays, s.samples + s.skipped_samples, s.shaded_samples, s.shadow_samples + s.skipped_shadow_samples, s.active_pixels)
    single = _start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(3, 6.0), skipping=True)
    whole = _render(ovr, single)
    ys, xs = np.mgrid[0:size[1], 0:size[0]]
    owner = ((xs // tw) + (ys // th)) % 3
    rgba, layer = np.zeros_like(whole[0]), np.zeros_like(whole[1])
    totals = np.zeros(5, np.int64)
    for rank in range(3):
        ren = hip_renderer_factory()
        ren.set_image_shard(rank, 3, tw, th)
        _start(ovr, ren, case, iso, MIXED, ao=(3, 6.0), skipping=True)
        part = _render(ovr, ren)
        rgba[owner == rank], layer[owner == rank] = part[0][owner == rank], part[1][owner == rank]
        totals += total(part[2])
        ren.close()
    assert _same(rgba, whole[0]) and _same(layer, whole[1]) and tuple(totals) == total(whole[2])
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        _start(ovr, group, case, iso, MIXED, ao=(3, 6.0), skipping=True)
        g = _render(ovr, group)
        s = group.get_ambient_occlusion()
        assert _same(g[0], whole[0]) and _same(g[1], whole[1]) and (s.samples, s.distance, s.active) == (3, 6.0, 1) and total(g[2]) == total(whole[2])
    finally:
        group.close()
    single.close()


@pytest.mark.parametrize("am", (0, 1, 2, 3))
def test_every_addressing_mode(ovr, oracle, hip_renderer_factory, monkeypatch, am):
    """every addressing mode the small volume can be forced into renders mode 0's frame"""
    vol = IC.volume("ball", np.uint16)
    iso = IC.scaled(IC.NESTED["ball"], np.uint16)
    case = _case(ovr, vol, shading=1)
    monkeypatch.setenv("OVR_HIP_ADDRESSING", "0")
    base = _start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(3, 6.0))
    want = _render(ovr, base)
    monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
    ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(3, 6.0))
    got = _render(ovr, ren)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and [getattr(got[2], k) for k in COUNTERS] == [getattr(want[2], k) for k in COUNTERS] and want[2].shaded_samples > 100, am
    ren.close()
    base.close()


# ---- 5. errors and state -----------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_state_intact_and_the_getter_reports_the_committed_state(ovr, hip_renderer_factory):
    import torch
    lib = ovr._lib.load()
    dev = torch.device("cuda", 0)
    buf = torch.zeros(8 + 8 * 16, dtype=torch.float32, device=dev)
    p = buf.data_ptr()
    empty = hip_renderer_factory()
    assert lib.ovr_hip_isosurface_ao_floats(empty._h, p, p, p, 1, 8, 0, 0) < 0 and b"no volume" in lib.ovr_hip_last_error()
    empty.close()
    case = _case(ovr, IC.volume("ball", np.float32))
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    assert lib.ovr_hip_isosurface_ao_floats(ren._h, p, p, p, 1, 8, 0, 0) < 0 and b"no isovalue" in lib.ovr_hip_last_error()
    ren.set_isosurfaces([0.5, 0.2], [0.25, 0.75])
    ren.commit()
    assert lib.ovr_hip_isosurface_ao_floats(ren._h, p, p, p, 1, 8, 0, 0) < 0 and b"no ambient-occlusion sample" in lib.ovr_hip_last_error()
    ren.set_ambient_occlusion(4, 5.0)
    s = ren.get_ambient_occlusion()
    assert (s.samples, s.distance, s.active) == (0, INF, 0), "the getter reports the committed state, not the queued one"
    assert ren.ambient_occlusion_directions().shape == (16, 0, 3)
    ren.commit()
    good = _render(ovr, ren)
    for K, R in ((-1, 1.0), (17, 1.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, -INF)):
        with pytest.raises(RuntimeError, match="ovr_hip_set_ambient_occlusion"):
            ren.set_ambient_occlusion(K, R)
    for args in ((None, p, p, 1, 8, 0, 0), (p, None, p, 1, 8, 0, 0), (p, p, None, 1, 8, 0, 0), (p, p, p, -1, 8, 0, 0), (p, p, p, 1, 0, 0, 0), (p, p, p, 1, 17, 0, 0), (p, p, p, 1, 8, -1, 0),
                 (p, p, p, 1, 8, 16, 0)):
        assert lib.ovr_hip_isosurface_ao_floats(ren._h, *args) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_isosurface_ao_floats(ren._h, p, p, p, 0, 8, 15, 1) == 0     # n == 0: nothing to do
    small = (np.zeros(3, F)).ctypes
    import ctypes as C
    assert lib.ovr_hip_get_ambient_occlusion_directions(ren._h, small.data_as(C.POINTER(C.c_float)), 3) < 0
    ren.commit()
    again = _render(ovr, ren)
    s = ren.get_ambient_occlusion()
    assert (s.samples, s.distance, s.rotations, s.active) == (4, 5.0, 16, 1)
    assert again[2].frame_index == good[2].frame_index + 1 and _same(again[1], good[1]) and again[2].shaded_samples == good[2].shaded_samples      # nothing was queued
    ren.set_ambient_occlusion(4, INF)
    ren.commit()
    assert ren.get_ambient_occlusion().distance == INF and _render(ovr, ren)[2].shadow_samples > good[2].shadow_samples
    ren.close()


# ---- 6. the other known-answer entries beside committed AO samples ----------------------------------------------------------------------------

def test_the_other_known_answer_entries_do_not_see_the_samples(ovr, hip_renderer_factory):
    dims = IC.DIMS[0]
    vol = IC.volume("smooth", np.float32, dims)
    org, d, _ = PC.ray_set(dims)
    pos = (np.random.default_rng(3).random((200, 3)) * np.array(dims)).astype(F)
    case = _case(ovr, vol)
    iso = IC.NESTED["smooth"]
    plain = _start(ovr, hip_renderer_factory(), case, iso, MIXED)
    plain.render()

    def entries(ren):
        out = [ren.isosurface_rays(org, d, skip) for skip in (False, True)] + [ren.isosurface_layer_rays(org, d, MAX_EVENTS, skip) for skip in (False, True)]
        return out, [ren.project_rays(org, d, mode, skip) for mode in (1, 2, 3) for skip in (False, True)], ren.shadow_floats(pos, 0)

    want = entries(plain)
    ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, ao=(8, 5.0))
    for name in ("committed, before a frame", "committed, behind an AO frame"):
        got = entries(ren)
        for a, b in zip(got[0], want[0]):
            assert all(np.array_equal(a[k], b[k]) if a[k].dtype != F else _same(a[k], b[k]) for k in b), name
        for a, b in zip(got[1], want[1]):
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name
        assert _same(got[2], want[2]), name
        assert _render(ovr, ren)[2].shadow_samples > plain.stats().shadow_samples
    ren.close()
    plain.close()


# ---- 7. the drop-in plugin ----------------------------------------------------------------------------------------------------------------------

def test_renderbatch_ao_variables(tmp_path, ovr, hip_renderer_factory):
    if not (os.path.exists(RENDERBATCH) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/renderbatch or plugin/libdevice_hip.so missing: they are built by __graft_entry__.build() where the reference tree is present and travel with the snapshot")
    from PIL import Image
    n, W, H = 32, 48, 36
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("dense", 256, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.25)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env.get("LD_LIBRARY_PATH", "")])
    env.pop("OVR_HIP_QUIET", None)
    env.update(OVR_HIP_ISOVALUES="0.7,0.4", OVR_HIP_AO_SAMPLES="4", OVR_HIP_AO_DISTANCE="6")
    out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / "ao")],
                         env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "[hip] ambient occlusion: 4 samples within 6" in out.stderr
    got = np.asarray(Image.open(str(tmp_path / "ao000000.png")).convert("RGBA"))
    scene, camera = ovr.vidi3d.scene_from_file(scene_path)

    def host(ao):
        ren = hip_renderer_factory()
        ren.set_fbsize((W, H))
        ren.set_frame_accumulation(True)
        ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
        ren.init(scene, camera)
        ren.set_camera(camera.eye, camera.at, camera.up)   # fovy 60 (renderer.h:149-152)
        ren.set_isosurfaces([0.7, 0.4])
        ren.set_empty_space_skipping(True)       # the plugin's default
        if ao:
            ren.set_ambient_occlusion(*ao)
        ren.commit()
        for _ in range(5 + 25):                  # main_batch.cpp:278-285: the saved frame is the mean of 30 accumulated ones
            ren.render()
        active = ren.get_ambient_occlusion().active
        img = np.array(ren.mapframe_rgba8(flip_vertical=True), copy=True).reshape(H, W, 4)
        ren.close()
        return img, active

    want, active = host((4, 6.0))
    plain, _ = host(None)
    assert active == 1 and np.array_equal(got, want) and want[..., 3].any() and not np.array_equal(want, plain)
