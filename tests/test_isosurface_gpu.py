"""Isosurfaces on the GPU (include/ovr_hip.h ovr_hip_set_isosurfaces) against the numpy model open-volume-renderer_amd/isosurface.py.
"Bits" are float32 bit patterns.  Hit, isovalue, t*, the steps walked and the shadow term involve no approximated operation: they are the model's bits in the
product build too (for u8 through isosurface.product_sampler, the product's 8-bit arithmetic).  The normal and the shade factor use the product's reciprocal
multiply and v_rsq_f32: helpers.compare's float bar there, bits under the exact-parity library (test_isosurfaces_are_exact_under_the_exact_parity_build)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

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


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, cam="oblique", rate=1.0, shading=2, spp=1, size=IC.SIZE):
    colors, alphas, vr = PC.transfer_function(ovr, "sparse", vol.dtype)
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=IC.BEHIND if cam == "behind" else IC.CAMERAS[cam], size=size, shading=shading, rate=rate, spp=spp, convention=0,
                spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=IC.FOVY)


def _start(ovr, ren, case, iso, skipping=False, accumulate=False):
    hip_setup(ovr, ren, case, accumulate=accumulate)
    ren.set_isosurfaces(iso)
    ren.set_empty_space_skipping(skipping)
    ren.commit()
    return ren


def _render(ovr, ren):
    ren.render()
    rgba, layer = hip_frame(ovr, ren)
    return rgba, layer, ren.stats()


def _sampler(ovr, vol):
    """the model's tap for the library under test: the product's 8-bit arithmetic unless the exact-parity build runs"""
    return None if EXACT_RUN else ovr.isosurface.product_sampler(vol)


_models = {}


def _model(ovr, oracle, case, iso, kind, **kw):
    """the model's frame of a case, computed once per key and shared"""
    key = (kind, np.dtype(case["vol"].dtype).name, case["vol"].shape, case["cam"], case["rate"], case["shading"], case["size"], tuple(float(x) for x in iso),
           tuple(sorted((k, str(v)) for k, v in kw.items() if k != "noise")))
    if key not in _models:
        I, P = ovr.isosurface, ovr.projection
        w, h = case["size"]
        basis = oracle.camera_basis(*case["cam"], case["fovy"], w, h).reshape(4, 3)
        ct, _ = PC.tables(case["colors"], case["alphas"])
        _models[key] = I.frame(case["vol"], basis, case["size"], case["rate"], iso, ct, P.normalized_range(case["vr"], case["vol"].dtype), shading=case["shading"],
                               sampler=_sampler(ovr, case["vol"]), **kw)
    return _models[key]


def _check_frame(oracle, case, got, want, name, skipping=False):
    rgba, layer, st = got
    ref, ref_layer, cnt = want
    assert _same(layer, ref_layer), (name, float(np.abs(layer - ref_layer).max()))
    if EXACT_RUN or case["shading"] == 0:
        assert _same(rgba, ref), (name, float(np.abs(rgba - ref).max()))
    else:
        compare(oracle, rgba, ref, name=str(name))
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"] and st.samples + st.skipped_samples == cnt["steps"] and st.shaded_samples == cnt["hits"], name
    assert st.shadow_samples + st.skipped_shadow_samples == cnt["shadow_steps"], name
    if not skipping:
        assert st.skipped_samples == 0 and st.skipped_shadow_samples == 0, name
    assert st.layout == 0 and st.pipeline == 1 and st.tuning == 0, name


# ---- 1. ovr_hip_isosurface_floats against the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("am", (0, 1, 2, 3))
def test_isosurface_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
    I = ovr.isosurface
    hits = 0
    for dims in IC.DIMS:
        vol = IC.volume("smooth", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        iso = IC.scaled(IC.NESTED["smooth"][1:], dtype)
        ren = hip_setup(ovr, hip_renderer_factory(), _case(ovr, vol))
        ren.set_light_direction(LIGHT, 1.0)
        ren.set_isosurfaces(iso[::-1])      # (stored ascending)
        ren.commit()
        assert list(ren.get_isosurfaces().isovalues[:3]) == list(iso) and ren.get_isosurfaces().n == 3
        for rate in IC.RATES:
            ren.set_volume_sampling_rate(rate)
            ren.commit()
            want = I.trace_rays(vol, org, d, rate, iso, light=LIGHT, sampler=_sampler(ovr, vol))
            for skip in (False, True):
                got = ren.isosurface_rays(org, d, skip)
                name = (am, dims, rate, skip)
                assert np.array_equal(got["hit"], want["hit"]) and np.array_equal(got["steps"], want["steps"]), name
                assert _same(got["iso"], want["iso"]) and _same(got["t"], want["t"]) and _same(got["shadow"], want["shadow"]), name
                if EXACT_RUN:
                    assert _same(got["normal"], want["normal"]), name
                else:
                    assert np.allclose(got["normal"], want["normal"], rtol=0, atol=TOL, equal_nan=True), (name, float(np.nanmax(np.abs(got["normal"] - want["normal"]))))
                assert not got["hit"][kind == "miss"].any() and (got["steps"][kind == "miss"] == 0).all()
            hits += int(want["hit"].sum())
        ren.close()
    assert hits > 40


# ---- 2. frames against the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", ("smooth", "ball"))
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, kind, dtype):
    vol = IC.volume(kind, dtype)
    iso = IC.scaled(IC.NESTED[kind][:2], dtype)
    for cam in sorted(IC.CAMERAS):
        for rate in IC.RATES:
            ren = None
            for shading in (2, 1, 0):
                case = _case(ovr, vol, cam=cam, rate=rate, shading=shading)
                if ren is None:
                    ren = hip_renderer_factory()
                    if cam == "axis":
                        ren.set_volume_layouts(2)     # thin replicas resident: an isosurface frame reads the general layout all the same
                    _start(ovr, ren, case, iso)
                else:
                    ren.set_shading(shading)
                    ren.commit()
                got = _render(ovr, ren)
                want = _model(ovr, oracle, case, iso, kind)
                _check_frame(oracle, case, got, want, (kind, cam, rate, shading))
                assert (got[1][..., 2] == 1).sum() > 40 and ren.get_isosurfaces().n == 2 and ren.get_isosurfaces().range_skipping == 0
                assert (got[2].shadow_samples > 0) == (shading == 2)
            ren.close()


def test_isosurfaces_are_exact_under_the_exact_parity_build():
    """started the way tests/test_projection_gpu.py starts its child: with the exact-parity build of the kernels normals, shade factors and the 8-bit volumes give the
    model's bits"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(isosurface_floats_vs_model and uint8) or (frames_vs_model and ball)"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 4 + 3 and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 3. the hit mask from the merged projections -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dtype", [("smooth", np.float32), ("plateau", np.uint8), ("twin", np.uint16), ("ball", np.uint8)], ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_hit_mask_from_the_projections(ovr, hip_renderer_factory, kind, dtype):
    """on ONE renderer, one sample per pixel, no jitter: hit == (v_max >= iso) & (v_min < iso) from the layers of a MAXIMUM and a MINIMUM frame, exactly"""
    vol = IC.volume(kind, dtype)
    for cam in sorted(IC.CAMERAS):
        case = _case(ovr, vol, cam=cam, rate=2.5, shading=0)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        layers = {}
        for mode in (1, 2):
            ren.set_projection(mode)
            ren.commit()
            layers[mode] = _render(ovr, ren)[1]
        marched = layers[1][..., 2] == 1
        for iso in IC.scaled(IC.ISOVALUES[kind], dtype):
            ren.set_isosurfaces([iso])       # the projection mode stays committed, and is not drawn
            ren.commit()
            got = _render(ovr, ren)
            want = marched & (layers[1][..., 0] >= iso) & (layers[2][..., 0] < iso)
            assert np.array_equal(got[1][..., 2] == 1, want), (kind, cam, float(iso))
            assert ren.get_projection().mode == 2 and (got[1][..., 0][want] == iso).all() and (got[0][..., 3] == want).all()
        ren.set_isosurfaces([])
        ren.commit()
        assert _same(_render(ovr, ren)[1], layers[2]), "the committed projection mode resumes"
        ren.close()


# ---- 4. range skipping is invisible ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dtype", [("slab", np.float32), ("slab", np.uint16), ("plateau", np.uint8), ("twin", np.uint8), ("ball", np.float32)],
                         ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_range_skipping_is_invisible(ovr, hip_renderer_factory, kind, dtype):
    vol = IC.volume(kind, dtype)
    iso = IC.scaled(IC.ISOVALUES[kind], dtype)
    skipped = 0
    for cam in sorted(IC.CAMERAS) + ["behind"]:
        case = _case(ovr, vol, cam=cam, rate=2.5, shading=2)
        plain, skipping = _start(ovr, hip_renderer_factory(), case, iso), _start(ovr, hip_renderer_factory(), case, iso, skipping=True)
        a, b = _render(ovr, plain), _render(ovr, skipping)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), (kind, cam)
        assert a[2].skipped_samples == 0 and a[2].samples == b[2].samples + b[2].skipped_samples and a[2].rays == b[2].rays and a[2].shaded_samples == b[2].shaded_samples, (kind, cam)
        assert a[2].skipped_shadow_samples == 0 and a[2].shadow_samples == b[2].shadow_samples + b[2].skipped_shadow_samples, (kind, cam)
        assert plain.get_isosurfaces().range_skipping == 0 and skipping.get_isosurfaces().range_skipping == 1 and b[2].skipping_kernels == 1 and a[2].skipping_kernels == 0
        skipped += b[2].skipped_samples
        print(f"{kind} {np.dtype(dtype).name} {cam}: {b[2].skipped_samples} of {a[2].samples} steps skipped, {b[2].skipped_shadow_samples} of {a[2].shadow_samples} shadow steps")
        if kind == "slab" and cam == "behind":      # (from the front a ray meets the slab in the first cell it enters: every cell on its way holds the isovalues)
            assert b[2].skipped_samples > 0
        plain.close()
        skipping.close()
    assert skipped > 0 or kind == "twin"      # (twin: every cell holds the whole range)


def test_update_volume_moves_a_cells_range_across_the_isovalue(ovr, hip_renderer_factory):
    vol = IC.volume("slab", np.float32)
    patch = np.full((3, 9, 11), 0.97, F)     # inside the dim cells behind the slab (z >= 15), whose ranges excluded the isovalue 0.5: four of them now hold it
    lower = (14, 12, 15)
    patched = vol.copy()
    patched[lower[2]:lower[2] + 3, lower[1]:lower[1] + 9, lower[0]:lower[0] + 11] = patch
    case = _case(ovr, vol, cam="behind", rate=2.5)
    iso = [0.5]
    ren = _start(ovr, hip_renderer_factory(), case, iso, skipping=True)
    before = _render(ovr, ren)
    ren.update_volume(patch, lower)
    after = _render(ovr, ren)
    plain_ren = _start(ovr, hip_renderer_factory(), dict(case, vol=patched), iso, skipping=False)
    plain = _render(ovr, plain_ren)
    assert _same(after[0], plain[0]) and _same(after[1], plain[1]) and not _same(after[1], before[1])
    assert after[2].samples + after[2].skipped_samples == plain[2].samples and after[2].shaded_samples == plain[2].shaded_samples and after[2].skipped_samples > 0
    assert before[2].skipped_samples > after[2].skipped_samples, "the cells the box touched are fetched now"
    assert (after[1][..., 1][after[1][..., 2] == 1] < before[1][..., 1][after[1][..., 2] == 1]).any(), "no ray hits the patch in front of the slab"
    for r in (ren, plain_ren):
        r.close()


# ---- 5. off changes nothing --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shading", (0, 1, 2))
def test_off_changes_nothing(ovr, hip_renderer_factory, shading):
    case = _case(ovr, PC.volume("smooth", np.float32), shading=shading, rate=1.0)
    never, off = hip_renderer_factory(), hip_renderer_factory()
    hip_setup(ovr, never, case)
    _start(ovr, off, case, [0.5])
    on = _render(ovr, off)
    assert on[2].shaded_samples > 0 and off.get_isosurfaces().n == 1
    off.set_isosurfaces([])
    off.commit()
    a, b = _render(ovr, never), _render(ovr, off)
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and not _same(on[0], b[0])
    assert [getattr(a[2], k) for k in COUNTERS] == [getattr(b[2], k) for k in COUNTERS] and a[2].pipeline == b[2].pipeline and a[2].layout == b[2].layout
    assert a[2].samples > 0 and off.get_isosurfaces().n == 0
    never.close()
    off.close()


# ---- 6. the downstream machinery ---------------------------------------------------------------------------------------------------------------

def _noise():
    return np.random.default_rng(77).random((16, 16, 64)).astype(F)


def test_accumulation_spp_and_both_jitters(ovr, oracle, hip_renderer_factory):
    vol = IC.volume("ball", np.float32)
    iso = IC.scaled(IC.NESTED["ball"][:2], np.float32)
    case = _case(ovr, vol, rate=1.0, shading=0)
    want = _model(ovr, oracle, case, iso, "ball")
    ren = _start(ovr, hip_renderer_factory(), case, iso, accumulate=True)
    one = _render(ovr, ren)
    two = _render(ovr, ren)
    assert two[2].frame_index == 2 and _same(one[0], want[0]) and _same(two[0], one[0]) and _same(two[1], one[1])   # (a + a) / 2 == a
    ren.set_isosurfaces(iso)               # every call resets the accumulation
    ren.commit()
    assert _render(ovr, ren)[2].frame_index == 1
    ren.close()
    # three samples per pixel under the blue-noise jitter, against the model
    case3 = _case(ovr, vol, rate=1.0, spp=3, shading=0)
    noise = _noise()
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    _start(ovr, ren, case3, iso)
    got = _render(ovr, ren)
    want3 = _model(ovr, oracle, case3, iso, "ball", spp=3, noise=noise, frame_index=1)
    _check_frame(oracle, case3, got, want3, "spp 3")
    assert not _same(got[0], want[0])
    edge = (got[1][..., 2] > 0) & (got[1][..., 2] < 1)
    assert edge.any(), "no pixel whose three samples disagree: the jitter did nothing"
    ren.close()
    # RandomTEA: the same rays in every renderer, other rays than the pixel centres', the hit flag a multiple of 1 / 3
    a, b = (_render(ovr, _start(ovr, hip_renderer_factory(), case3, iso)) for _ in range(2))
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and not _same(a[0], want[0]) and a[2].rays == 3 * IC.SIZE[0] * IC.SIZE[1]
    assert np.isin(np.round(a[1][..., 2] * 3), (0, 1, 2, 3)).all() and np.abs(a[1][..., 2] * 3 - np.round(a[1][..., 2] * 3)).max() < 1e-6


def test_sparse_sampling_and_reconstruction(ovr, hip_renderer_factory):
    case = _case(ovr, IC.volume("ball", np.float32), rate=1.0)
    ren = hip_renderer_factory()
    ren.set_noise_tile(_noise())
    _start(ovr, ren, case, [0.35])
    dense = _render(ovr, ren)
    ren.set_sparse_sampling(True)
    ren.set_focus((0.5, 0.5), 0.3, 0.2)
    ren.commit()
    sparse = _render(ovr, ren)
    xy = ren.sparse_mask(sparse[2].frame_index).reshape(-1, 2)
    mask = np.zeros(dense[0].shape[:2], bool)
    mask[xy[:, 1], xy[:, 0]] = True
    assert 50 < mask.sum() < mask.size - 50 and sparse[2].active_pixels == mask.sum()
    assert _same(sparse[0][mask], dense[0][mask]) and _same(sparse[1][mask], dense[1][mask])
    assert not sparse[0][~mask].any() and not sparse[1][~mask].any()
    ren.set_reconstruction(1)
    ren.commit()
    filled = _render(ovr, ren)
    xy = ren.sparse_mask(filled[2].frame_index).reshape(-1, 2)
    mask[:] = False
    mask[xy[:, 1], xy[:, 0]] = True
    assert _same(filled[0][mask], dense[0][mask]) and _same(filled[1][mask], dense[1][mask]) and ren.reconstruction().valid == 1
    assert filled[0][~mask].any()
    ren.close()


def test_clip_box(ovr, oracle, hip_renderer_factory):
    vol = IC.volume("ball", np.float32)
    nz, ny, nx = vol.shape
    case = _case(ovr, vol, rate=2.5, shading=2)
    iso = [0.35]
    lower, upper = (5.5, -INF, 3.0), (19.0, 20.25, INF)      # cuts the ball open: the cut is no surface, rays enter the solid and hit where they leave it
    inv, wp = ovr.clipping.volume_constants((nx, ny, nz))
    box = ovr.clipping.object_box(lower, upper, inv, wp)
    for skip in (False, True):
        ren = _start(ovr, hip_renderer_factory(), case, iso, skipping=skip)
        unclipped = _render(ovr, ren)
        ren.set_clip_box(lower, upper)
        ren.commit()
        got = _render(ovr, ren)
        _check_frame(oracle, case, got, _model(ovr, oracle, case, iso, "ball", clip=box, skipping=skip), ("clip", skip), skipping=skip)
        assert not _same(got[1], unclipped[1])
        ren.set_clip_box((10.0, 0.0, 0.0), (10.0, 33.0, 18.0))   # empty
        ren.commit()
        empty = _render(ovr, ren)
        assert not empty[0].any() and not empty[1].any() and empty[2].samples == 0 and empty[2].shaded_samples == 0 and empty[2].rays == IC.SIZE[0] * IC.SIZE[1]
        ren.close()


def test_image_shards_and_device_group(ovr, hip_renderer_factory):
    size, tw, th = (56, 40), 16, 8
    case = _case(ovr, IC.volume("ball", np.float32), cam="oblique", rate=1.0, size=size)
    iso = [0.2, 0.5]
    total = lambda s: (s.rays, s.samples + s.skipped_samples, s.shaded_samples, s.shadow_samples + s.skipped_shadow_samples, s.active_pixels)
    single = _start(ovr, hip_renderer_factory(), case, iso, skipping=True)
    whole = _render(ovr, single)
    ys, xs = np.mgrid[0:size[1], 0:size[0]]
    owner = ((xs // tw) + (ys // th)) % 3
    rgba, layer = np.zeros_like(whole[0]), np.zeros_like(whole[1])
    totals = np.zeros(5, np.int64)
    for rank in range(3):
        ren = hip_renderer_factory()
        ren.set_image_shard(rank, 3, tw, th)
        _start(ovr, ren, case, iso, skipping=True)
        part = _render(ovr, ren)
        rgba[owner == rank], layer[owner == rank] = part[0][owner == rank], part[1][owner == rank]
        totals += total(part[2])
        ren.close()
    assert _same(rgba, whole[0]) and _same(layer, whole[1]) and tuple(totals) == total(whole[2])
    group = ovr.create_renderer("hip", devices=[0, 0])
    try:
        _start(ovr, group, case, iso, skipping=True)
        g = _render(ovr, group)
        assert _same(g[0], whole[0]) and _same(g[1], whole[1]) and group.get_isosurfaces().n == 2 and total(g[2]) == total(whole[2])
    finally:
        group.close()
    single.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_state_intact(ovr, hip_renderer_factory):
    import ctypes as C
    import torch
    lib = ovr._lib.load()
    dev = torch.device("cuda", 0)
    buf = torch.zeros(24, dtype=torch.float32, device=dev)
    empty = hip_renderer_factory()
    assert lib.ovr_hip_isosurface_floats(empty._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 0) < 0 and b"no volume" in lib.ovr_hip_last_error()
    empty.close()
    case = _case(ovr, IC.volume("ball", np.float32))
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    assert lib.ovr_hip_isosurface_floats(ren._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 0) < 0 and b"no isovalue" in lib.ovr_hip_last_error()
    ren.set_isosurfaces([0.5, 0.2])
    ren.commit()
    good = _render(ovr, ren)
    four = (C.c_float * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    for bad in ([0.1, 0.2, 0.3, 0.4, 0.5], [np.nan], [0.1, np.inf], [-np.inf], [0.3, 0.1, 0.3]):
        with pytest.raises(RuntimeError, match="ovr_hip_set_isosurfaces"):
            ren.set_isosurfaces(bad)
    assert lib.ovr_hip_set_isosurfaces(ren._h, four, -1) < 0 and lib.ovr_hip_set_isosurfaces(ren._h, four, 5) < 0 and lib.ovr_hip_set_isosurfaces(ren._h, None, 2) < 0
    for args in ((None, buf.data_ptr(), buf.data_ptr(), 1, 0), (buf.data_ptr(), None, buf.data_ptr(), 1, 0), (buf.data_ptr(), buf.data_ptr(), None, 1, 0),
                 (buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), -1, 0)):
        assert lib.ovr_hip_isosurface_floats(ren._h, *args) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_isosurface_floats(ren._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 0) == 0     # n == 0: nothing to do
    ren.commit()
    again = _render(ovr, ren)
    s = ren.get_isosurfaces()
    assert s.n == 2 and list(s.isovalues) == [F(0.2), F(0.5), 0.0, 0.0] and again[2].frame_index == good[2].frame_index + 1      # nothing was queued: no reset
    assert _same(again[0], good[0]) and _same(again[1], good[1]) and again[2].samples == good[2].samples
    ren.close()


# ---- 8. the other known-answer entries beside committed isovalues ------------------------------------------------------------------------------

def test_project_and_shadow_floats_do_not_see_the_isovalues(ovr, hip_renderer_factory):
    """ovr_hip_project_floats and ovr_hip_shadow_floats copy the last frame's parameters: with isovalues committed and an isosurface frame rendered, and again right
    after n = 0 is committed and before any frame is rendered, they return what a renderer that never called the setter returns, bit for bit"""
    dims = IC.DIMS[0]
    vol = IC.volume("smooth", np.float32, dims)
    org, d, _ = PC.ray_set(dims)
    pos = (np.random.default_rng(3).random((200, 3)) * np.array(dims)).astype(F)
    case = _case(ovr, vol)
    never = hip_setup(ovr, hip_renderer_factory(), case)
    never.render()
    want = [never.project_rays(org, d, mode, skip) for mode in (1, 2, 3) for skip in (False, True)]
    want_shadow = never.shadow_floats(pos, 0)
    never.set_shadow_cache(1, 4)
    never.commit()
    want_lookup = never.shadow_floats(pos, 1)
    assert (want_shadow > 0).any() and (want[0][2] > 0).any()

    def check(ren, name):
        got = [ren.project_rays(org, d, mode, skip) for mode in (1, 2, 3) for skip in (False, True)]
        for a, b in zip(got, want):
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name
        assert _same(ren.shadow_floats(pos, 0), want_shadow), name

    ren = _start(ovr, hip_renderer_factory(), case, [0.45, 0.6])
    check(ren, "committed, before a frame")
    on = _render(ovr, ren)
    assert on[2].shaded_samples > 0
    check(ren, "committed, behind an isosurface frame")
    ren.set_shadow_cache(1, 4)      # the lattice is built through the same launch helper, from the isosurface frame's parameters
    ren.commit()
    assert _same(ren.shadow_floats(pos, 1), want_lookup), "the lattice built beside committed isovalues"
    ren.set_shadow_cache(0)
    ren.set_isosurfaces([])
    ren.commit()
    check(ren, "n = 0 committed, no frame rendered since")
    assert ren.get_isosurfaces().n == 0
    ren.close()
    never.close()


# ---- 9. non-finite voxels ----------------------------------------------------------------------------------------------------------------------

def test_nonfinite_voxels_follow_the_model_and_fault_nowhere(ovr, oracle, hip_renderer_factory):
    """NaN, +Inf and -Inf voxels: without skipping hit, isovalue, t*, steps walked and the shadow term are the model's bits (a NaN sample has side 0, a NaN secant
    clamps to the interval's start); with skipping a frame and the rays complete, every flag is 0 or 1 and nothing is NaN where nothing may be"""
    I = ovr.isosurface
    dims = IC.DIMS[0]
    vol = IC.nonfinite_volume(dims)
    assert np.isnan(vol).sum() >= 8 and np.isinf(vol).sum() >= 16
    org, d, _ = PC.ray_set(dims)
    iso = IC.scaled(IC.NESTED["smooth"][1:], np.float32)
    ren = _start(ovr, hip_renderer_factory(), _case(ovr, vol, rate=2.5), iso)
    clean = I.trace_rays(IC.volume("smooth", np.float32, dims), org, d, 2.5, iso)
    for rate in IC.RATES:
        ren.set_volume_sampling_rate(rate)
        ren.commit()
        want = I.trace_rays(vol, org, d, rate, iso)
        got = ren.isosurface_rays(org, d, False)
        assert np.array_equal(got["hit"], want["hit"]) and np.array_equal(got["steps"], want["steps"]), rate
        assert _same(got["iso"], want["iso"]) and _same(got["t"], want["t"]) and _same(got["shadow"], want["shadow"]), rate
        fin = want["hit"] & np.isfinite(want["normal"]).all(1)
        assert np.allclose(got["normal"][fin], want["normal"][fin], rtol=0, atol=TOL), rate
        skipped = ren.isosurface_rays(org, d, True)
        assert set(np.unique(skipped["shadow"])) <= {0.0, 1.0} and np.isfinite(skipped["t"]).all() and (skipped["steps"] >= 0).all()
    assert (_bits(want["t"]) != _bits(clean["t"])).sum() >= 4, "the non-finite voxels touch too few rays of the set"
    for skip in (False, True):
        ren.set_empty_space_skipping(skip)
        ren.commit()
        rgba, layer, st = _render(ovr, ren)
        assert st.rays == IC.SIZE[0] * IC.SIZE[1] and np.isin(layer[..., 2], (0.0, 1.0)).all() and np.isfinite(layer).all() and np.isin(rgba[..., 3], (0.0, 1.0)).all()
        assert st.shaded_samples == int(layer[..., 2].sum()) > 20
        if not skip:      # the layer and the counters are the model's; the colours are not NaN anywhere (clamp01 turns a NaN shade into 0)
            case = _case(ovr, vol, rate=IC.RATES[-1])
            ref, ref_layer, cnt = _model(ovr, oracle, case, iso, "nonfinite")
            assert _same(layer, ref_layer) and not np.isnan(rgba).any() and st.samples == cnt["steps"] and st.shadow_samples == cnt["shadow_steps"]
    ren.close()


# ---- 10. the drop-in plugin ---------------------------------------------------------------------------------------------------------------------

def test_renderbatch_isovalues_variable(tmp_path, ovr, oracle, hip_renderer_factory):
    if not (os.path.exists(RENDERBATCH) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/renderbatch or plugin/libdevice_hip.so missing: they are built by __graft_entry__.build() where the reference tree is present and travel with the snapshot")
    from PIL import Image
    n, W, H = 40, 96, 64
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("dense", 256, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.25)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env.get("LD_LIBRARY_PATH", "")])
    env.pop("OVR_HIP_QUIET", None)
    env["OVR_HIP_ISOVALUES"] = "0.7,0.4"
    out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / "iso")],
                         env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "[hip] isosurfaces at 0.7, 0.4" in out.stderr
    got = np.asarray(Image.open(str(tmp_path / "iso000000.png")).convert("RGBA"))
    scene, camera = ovr.vidi3d.scene_from_file(scene_path)
    ren = hip_renderer_factory()
    ren.set_fbsize((W, H))
    ren.set_frame_accumulation(True)
    ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
    ren.init(scene, camera)
    ren.set_camera(camera.eye, camera.at, camera.up)   # fovy 60 (renderer.h:149-152)
    ren.set_isosurfaces([0.7, 0.4])
    ren.set_empty_space_skipping(True)       # the plugin's default
    ren.commit()
    for _ in range(5 + 25):                  # main_batch.cpp:278-285: the saved frame is the mean of 30 accumulated ones
        ren.render()
    assert ren.stats().shaded_samples > 0 and ren.stats().frame_index == 30 and ren.get_isosurfaces().n == 2
    want = np.array(ren.mapframe_rgba8(flip_vertical=True), copy=True).reshape(H, W, 4)
    assert np.array_equal(got, want) and want[..., 3].any()
    # the model's frame of the same scene: its hit mask is the saved image's opaque pixels, exactly (a = 1 on a hit, 0 on a miss; the PNG is flipped)
    basis = oracle.camera_basis(camera.eye, camera.at, camera.up, 60.0, W, H).reshape(4, 3)
    model = ovr.isosurface.frame(vol, basis, (W, H), 1.0, [0.4, 0.7], np.ones((2, 3), F), (F(0.0), F(1.0)), shading=ovr.isosurface.NONE)      # (the mask: any colours)
    assert np.array_equal(got[::-1, :, 3] == 255, model[1][..., 2] == 1) and 100 < (model[1][..., 2] == 1).sum() < W * H - 100
    ren.close()
