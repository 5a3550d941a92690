"""Translucent isosurfaces on the GPU (include/ovr_hip.h ovr_hip_set_isosurface_layers) against the numpy model
open-volume-renderer_amd/isosurface.py.  "Bits" are float32 bit patterns.  Events, k, t*, A, the shadow term, the layer, the steps and the counters involve no
approximated operation: they are the model's bits in the product build too (for u8 through isosurface.product_sampler).  Normals and colours use the product's
reciprocal multiply and v_rsq_f32: helpers.compare's float bar there (atol 2e-4 on normals), bits under the exact-parity library
(test_layers_are_exact_under_the_exact_parity_build)."""
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
MIXED, THIN = (0.3, 0.4, 0.5, 1.0), (0.3, 0.3, 0.3, 0.3)     # MIXED: rays that reach the innermost shell end there, early
OPACITIES = {"ball": MIXED, "smooth": THIN}
UNREACHABLE = 1.0e9
MAX_EVENTS = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, cam="oblique", rate=1.0, shading=2, spp=1, size=IC.SIZE):
    colors, alphas, vr = PC.transfer_function(ovr, "sparse", vol.dtype)
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=IC.BEHIND if cam == "behind" else IC.CAMERAS[cam], size=size, shading=shading, rate=rate, spp=spp, convention=0,
                spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=IC.FOVY)


def _start(ovr, ren, case, iso, opacities, skipping=False, accumulate=False):
    hip_setup(ovr, ren, case, accumulate=accumulate)
    ren.set_isosurfaces(iso, opacities)
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


def _model(ovr, oracle, case, iso, opacities, kind, **kw):
    """the model's frame of a case, computed once per key and shared"""
    key = (kind, np.dtype(case["vol"].dtype).name, case["vol"].shape, case["cam"], case["rate"], case["shading"], case["size"], tuple(float(x) for x in iso),
           None if opacities is None else tuple(float(x) for x in opacities), tuple(sorted((k, str(v)) for k, v in kw.items() if k != "noise")))
    if key not in _models:
        I, P = ovr.isosurface, ovr.projection
        w, h = case["size"]
        basis = oracle.camera_basis(*case["cam"], case["fovy"], w, h).reshape(4, 3)
        ct, _ = PC.tables(case["colors"], case["alphas"])
        _models[key] = I.frame(case["vol"], basis, case["size"], case["rate"], iso, ct, P.normalized_range(case["vr"], case["vol"].dtype), shading=case["shading"],
                               sampler=_sampler(ovr, case["vol"]), opacities=opacities, **kw)
    return _models[key]


def _check_frame(oracle, case, got, want, name, skipping=False):
    rgba, layer, st = got
    ref, ref_layer, cnt = want
    assert _same(layer, ref_layer), (name, float(np.abs(layer - ref_layer).max()))
    assert _same(rgba[..., 3], ref[..., 3]), (name, "A", float(np.abs(rgba[..., 3] - ref[..., 3]).max()))
    if EXACT_RUN or case["shading"] == 0:
        assert _same(rgba, ref), (name, float(np.abs(rgba - ref).max()))
    else:
        compare(oracle, rgba, ref, name=str(name))
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"] and st.samples + st.skipped_samples == cnt["steps"] and st.shaded_samples == cnt["hits"], \
        (name, st.samples + st.skipped_samples, cnt["steps"], st.shaded_samples, cnt["hits"])
    assert st.shadow_samples + st.skipped_shadow_samples == cnt["shadow_steps"], (name, st.shadow_samples + st.skipped_shadow_samples, cnt["shadow_steps"])
    if not skipping:
        assert st.skipped_samples == 0 and st.skipped_shadow_samples == 0, name
    assert st.layout == 0 and st.pipeline == 1 and st.tuning == 0, name


def _check_rays(got, want, name):
    """ovr_hip_isosurface_layers_floats against trace_rays(opacities=...)"""
    n = len(want["n_events"])
    assert np.array_equal(got["events"], want["n_events"]) and _same(got["A"], want["A"]), name
    assert np.array_equal(got["steps"], want["steps"]) and np.array_equal(got["shadow_steps"], want["shadow_steps"]), name
    f = want["flat"]
    first = np.concatenate([[0], np.cumsum(want["n_events"])[:-1]])
    slot = np.arange(len(f["ray"])) - first[f["ray"]]
    keep = slot < MAX_EVENTS
    r, e = f["ray"][keep], slot[keep]
    assert np.array_equal(got["k"][r, e], f["k"][keep]), name
    for key, mine in (("t", "t"), ("shadow", "shadow"), ("A_after", "A")):
        assert _same(got[key][r, e], f[mine][keep]), (name, key)
    if EXACT_RUN:
        assert _same(got["normal"][r, e], f["normal"][keep]), name
    else:
        assert np.allclose(got["normal"][r, e], f["normal"][keep], rtol=0, atol=TOL, equal_nan=True), (name, float(np.nanmax(np.abs(got["normal"][r, e] - f["normal"][keep]))))
    empty = np.ones((n, MAX_EVENTS), bool)
    empty[r, e] = False
    assert not got["t"][empty].any() and not got["A_after"][empty].any() and not got["normal"][empty].any() and not got["k"][empty].any(), (name, "the rest is zeros")


# ---- 1. ovr_hip_isosurface_layers_floats against the model ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("am", (0, 1, 2, 3))
def test_layer_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
    I = ovr.isosurface
    events = deep = early = 0
    for dims in IC.DIMS:
        vol = IC.volume("ball", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        iso = IC.scaled(IC.NESTED["ball"], dtype)
        ren = hip_setup(ovr, hip_renderer_factory(), _case(ovr, vol))
        ren.set_light_direction(LIGHT, 1.0)
        ren.set_isosurfaces(iso[::-1], MIXED[::-1])      # (stored ascending, the opacities with their isovalues)
        ren.commit()
        s = ren.get_isosurface_layers()
        assert list(s.isovalues) == list(iso) and list(s.opacities) == [F(a) for a in MIXED] and s.n == 4 and s.translucent == 1
        for rate in IC.RATES:
            ren.set_volume_sampling_rate(rate)
            ren.commit()
            want = I.trace_rays(vol, org, d, rate, iso, light=LIGHT, sampler=_sampler(ovr, vol), opacities=MIXED)
            for skip in (False, True):
                got = ren.isosurface_layer_rays(org, d, MAX_EVENTS, skip)
                _check_rays(got, want, (am, dims, rate, skip))
                assert not got["events"][kind == "miss"].any() and (got["steps"][kind == "miss"] == 0).all()
            events += int(want["n_events"].sum())
            deep += int((want["n_events"] >= 4).sum())
            early += int((want["A"] == 1).sum())
        ren.close()
    assert events > 200 and deep > 20 and early > 10, (events, deep, early)


# ---- 2. frames against the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", ("smooth", "ball"))
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, kind, dtype):
    I = ovr.isosurface
    vol = IC.volume(kind, dtype)
    iso = IC.scaled(IC.NESTED[kind], dtype)
    op = OPACITIES[kind]
    for cam in sorted(IC.CAMERAS):
        for rate in IC.RATES:
            ren = None
            for shading in (2, 1, 0):
                case = _case(ovr, vol, cam=cam, rate=rate, shading=shading)
                if ren is None:
                    ren = _start(ovr, hip_renderer_factory(), case, iso, op)
                    w, h = case["size"]
                    basis = oracle.camera_basis(*case["cam"], case["fovy"], w, h).reshape(4, 3)
                    dirs = ovr.projection.pixel_rays(basis, w, h, None).reshape(-1, 3)
                    ne = I.trace_rays(vol, np.broadcast_to(basis[0], dirs.shape), dirs, rate, iso, shadows=False, sampler=_sampler(ovr, vol), opacities=op)["n_events"]
                    assert (ne >= 2).sum() >= 40 and (ne >= 4).sum() >= 30, (kind, cam, rate, int((ne >= 2).sum()), int((ne >= 4).sum()))
                else:
                    ren.set_shading(shading)
                    ren.commit()
                got = _render(ovr, ren)
                want = _model(ovr, oracle, case, iso, op, kind)
                _check_frame(oracle, case, got, want, (kind, cam, rate, shading))
                s = ren.get_isosurface_layers()
                assert s.n == 4 and s.translucent == 1 and s.range_skipping == 0 and got[2].shaded_samples == int(ne.sum())
                assert (got[2].shadow_samples > 0) == (shading == 2)
                a = got[0][..., 3]
                assert ((a > 0) & (a < 1)).sum() > 10, "no translucent pixel"
            ren.close()


def test_layers_are_exact_under_the_exact_parity_build():
    """started the way test_isosurfaces_are_exact_under_the_exact_parity_build starts its child: with the exact-parity build of the kernels normals, shade factors,
    colours and the 8-bit volumes give the model's bits"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(layer_floats_vs_model and uint8) or (frames_vs_model and ball)"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 4 + 3 and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 3. identities -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shading", (0, 2))
def test_all_ones_and_a_hidden_translucent_level_are_the_opaque_frame(ovr, hip_renderer_factory, shading):
    vol = IC.volume("ball", np.float32)
    iso = IC.scaled(IC.NESTED["ball"][:2], np.float32)
    case = _case(ovr, vol, rate=2.5, shading=shading)
    opaque = _start(ovr, hip_renderer_factory(), case, iso, None, skipping=True)
    want = _render(ovr, opaque)
    assert want[2].shaded_samples > 40
    ones = _start(ovr, hip_renderer_factory(), case, iso, (1.0, 1.0), skipping=True)
    got = _render(ovr, ones)
    s = ones.get_isosurface_layers()
    assert s.translucent == 0 and list(s.opacities) == [1.0, 1.0, 0.0, 0.0] and s.n == 2 and s.range_skipping == 1 and ones.get_isosurfaces().n == 2
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and [getattr(got[2], k) for k in COUNTERS] == [getattr(want[2], k) for k in COUNTERS]
    # one reachable level of opacity 1 beside a translucent one no sample reaches: the translucent kernel, the opaque frame and counters
    for skipping in (False, True):
        single = _start(ovr, hip_renderer_factory(), case, iso[:1], None, skipping=skipping)
        hidden = _start(ovr, hip_renderer_factory(), case, (iso[0], UNREACHABLE), (1.0, 0.5), skipping=skipping)
        a, b = _render(ovr, single), _render(ovr, hidden)
        assert hidden.get_isosurface_layers().translucent == 1 and single.get_isosurface_layers().translucent == 0
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and [getattr(a[2], k) for k in COUNTERS] == [getattr(b[2], k) for k in COUNTERS], skipping
        single.close()
        hidden.close()
    opaque.close()
    ones.close()


# ---- 4. range skipping is invisible ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dtype", [("ball", np.float32), ("smooth", np.uint16), ("ball", np.uint8)], ids=lambda x: x if isinstance(x, str) else np.dtype(x).name)
def test_range_skipping_is_invisible(ovr, hip_renderer_factory, kind, dtype):
    vol = IC.volume(kind, dtype)
    iso = IC.scaled(IC.NESTED[kind], dtype)
    skipped = 0
    for cam in sorted(IC.CAMERAS):
        case = _case(ovr, vol, cam=cam, rate=2.5, shading=2)
        plain, skipping = _start(ovr, hip_renderer_factory(), case, iso, OPACITIES[kind]), _start(ovr, hip_renderer_factory(), case, iso, OPACITIES[kind], skipping=True)
        a, b = _render(ovr, plain), _render(ovr, skipping)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), (kind, cam)
        assert a[2].skipped_samples == 0 and a[2].samples == b[2].samples + b[2].skipped_samples and a[2].rays == b[2].rays and a[2].shaded_samples == b[2].shaded_samples, (kind, cam)
        assert a[2].skipped_shadow_samples == 0 and a[2].shadow_samples == b[2].shadow_samples + b[2].skipped_shadow_samples, (kind, cam)
        assert plain.get_isosurface_layers().range_skipping == 0 and skipping.get_isosurface_layers().range_skipping == 1 and b[2].skipping_kernels == 1 and a[2].skipping_kernels == 0
        skipped += b[2].skipped_samples + b[2].skipped_shadow_samples
        plain.close()
        skipping.close()
    assert skipped > 0


def test_range_skipping_behind_update_volume(ovr, hip_renderer_factory):
    vol = IC.volume("slab", np.float32)
    patch = np.full((3, 9, 11), 0.97, F)     # inside the dim cells behind the slab (z >= 15), whose ranges excluded the isovalues: four of them now hold them
    lower = (14, 12, 15)
    patched = vol.copy()
    patched[lower[2]:lower[2] + 3, lower[1]:lower[1] + 9, lower[0]:lower[0] + 11] = patch
    case = _case(ovr, vol, cam="behind", rate=2.5)
    iso, op = [0.5, 0.8], (0.4, 0.6)
    ren = _start(ovr, hip_renderer_factory(), case, iso, op, skipping=True)
    before = _render(ovr, ren)
    ren.update_volume(patch, lower)
    after = _render(ovr, ren)
    plain_ren = _start(ovr, hip_renderer_factory(), dict(case, vol=patched), iso, op, skipping=False)
    plain = _render(ovr, plain_ren)
    assert _same(after[0], plain[0]) and _same(after[1], plain[1]) and not _same(after[1], before[1])
    assert after[2].samples + after[2].skipped_samples == plain[2].samples and after[2].shaded_samples == plain[2].shaded_samples and after[2].skipped_samples > 0
    assert after[2].shadow_samples + after[2].skipped_shadow_samples == plain[2].shadow_samples and before[2].skipped_samples > after[2].skipped_samples
    for r in (ren, plain_ren):
        r.close()


# ---- 5. the downstream machinery ---------------------------------------------------------------------------------------------------------------

def _noise():
    return np.random.default_rng(77).random((16, 16, 64)).astype(F)


def test_accumulation_spp_and_both_jitters(ovr, oracle, hip_renderer_factory):
    vol = IC.volume("ball", np.float32)
    iso = IC.scaled(IC.NESTED["ball"], np.float32)
    case = _case(ovr, vol, rate=1.0, shading=0)
    want = _model(ovr, oracle, case, iso, MIXED, "ball")
    ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, accumulate=True)
    one = _render(ovr, ren)
    two = _render(ovr, ren)
    assert two[2].frame_index == 2 and _same(one[0], want[0]) and _same(two[0], one[0]) and _same(two[1], one[1])   # (a + a) / 2 == a
    ren.set_isosurfaces(iso, MIXED)               # every call resets the accumulation
    ren.commit()
    assert _render(ovr, ren)[2].frame_index == 1
    ren.close()
    # two samples per pixel under the blue-noise jitter, against the model
    case2 = _case(ovr, vol, rate=1.0, spp=2, shading=0)
    noise = _noise()
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    _start(ovr, ren, case2, iso, MIXED)
    got = _render(ovr, ren)
    want2 = _model(ovr, oracle, case2, iso, MIXED, "ball", spp=2, noise=noise, frame_index=1)
    _check_frame(oracle, case2, got, want2, "spp 2")
    assert not _same(got[0], want[0])
    edge = (got[1][..., 2] > 0) & (got[1][..., 2] < 1)
    assert edge.any(), "no pixel whose two samples disagree: the jitter did nothing"
    ren.close()
    # RandomTEA: the same rays in every renderer, other rays than the pixel centres'
    a, b = (_render(ovr, _start(ovr, hip_renderer_factory(), case2, iso, MIXED)) for _ in range(2))
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and not _same(a[0], want[0]) and a[2].rays == 2 * IC.SIZE[0] * IC.SIZE[1]
    assert np.isin(a[1][..., 2], (0.0, 0.5, 1.0)).all()


def test_sparse_sampling_and_reconstruction(ovr, hip_renderer_factory):
    case = _case(ovr, IC.volume("ball", np.float32), rate=1.0)
    ren = hip_renderer_factory()
    ren.set_noise_tile(_noise())
    _start(ovr, ren, case, IC.NESTED["ball"], MIXED)
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
    iso = IC.scaled(IC.NESTED["ball"], np.float32)
    lower, upper = (5.5, -INF, 3.0), (19.0, 20.25, INF)      # cuts the shells open: the cut is no surface, rays enter the solid and meet the shells from inside
    inv, wp = ovr.clipping.volume_constants((nx, ny, nz))
    box = ovr.clipping.object_box(lower, upper, inv, wp)
    for skip in (False, True):
        ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, skipping=skip)
        unclipped = _render(ovr, ren)
        ren.set_clip_box(lower, upper)
        ren.commit()
        got = _render(ovr, ren)
        _check_frame(oracle, case, got, _model(ovr, oracle, case, iso, MIXED, "ball", clip=box, skipping=skip), ("clip", skip), skipping=skip)
        assert not _same(got[1], unclipped[1])
        ren.set_clip_box((10.0, 0.0, 0.0), (10.0, 33.0, 18.0))   # empty
        ren.commit()
        empty = _render(ovr, ren)
        assert not empty[0].any() and not empty[1].any() and empty[2].samples == 0 and empty[2].shaded_samples == 0 and empty[2].rays == IC.SIZE[0] * IC.SIZE[1]
        ren.close()


def test_orthographic_camera(ovr, oracle, hip_renderer_factory):
    K, I, P = ovr.camera, ovr.isosurface, ovr.projection
    vol = IC.volume("ball", np.float32)
    iso = IC.scaled(IC.NESTED["ball"], np.float32)
    w, h = IC.SIZE
    for shading in (2, 0):
        for skip in (False, True):
            case = _case(ovr, vol, rate=1.0, shading=shading)
            ren = _start(ovr, hip_renderer_factory(), case, iso, MIXED, skipping=skip)
            ren.set_camera(ovr.Camera(*IC.CAMERAS["oblique"], orthographic_height=30.0))
            ren.commit()
            c = ren.get_camera()
            basis = tuple(np.array(list(v), F) for v in (c.pos, c.dir, c.hor, c.ver))
            ct, _ = PC.tables(case["colors"], case["alphas"])
            want = I.frame(vol, basis, (w, h), 1.0, iso, ct, P.normalized_range(case["vr"], vol.dtype), shading=shading, skipping=skip, camera_kind=K.ORTHOGRAPHIC, opacities=MIXED)
            got = _render(ovr, ren)
            _check_frame(oracle, case, got, want, ("orthographic", shading, skip), skipping=skip)
            assert want[2]["hits"] > 150 and ((got[0][..., 3] > 0) & (got[0][..., 3] < 1)).sum() > 10
            ren.close()


def test_image_shards_and_device_group(ovr, hip_renderer_factory):
    size, tw, th = (56, 40), 16, 8
    case = _case(ovr, IC.volume("ball", np.float32), cam="oblique", rate=1.0, size=size)
    iso = IC.NESTED["ball"]
    total = lambda s: (s.rays, s.samples + s.skipped_samples, s.shaded_samples, s.shadow_samples + s.skipped_shadow_samples, s.active_pixels)
    single = _start(ovr, hip_renderer_factory(), case, iso, MIXED, skipping=True)
    whole = _render(ovr, single)
    ys, xs = np.mgrid[0:size[1], 0:size[0]]
    owner = ((xs // tw) + (ys // th)) % 3
    rgba, layer = np.zeros_like(whole[0]), np.zeros_like(whole[1])
    totals = np.zeros(5, np.int64)
    for rank in range(3):
        ren = hip_renderer_factory()
        ren.set_image_shard(rank, 3, tw, th)
        _start(ovr, ren, case, iso, MIXED, skipping=True)
        part = _render(ovr, ren)
        rgba[owner == rank], layer[owner == rank] = part[0][owner == rank], part[1][owner == rank]
        totals += total(part[2])
        ren.close()
    assert _same(rgba, whole[0]) and _same(layer, whole[1]) and tuple(totals) == total(whole[2])
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        _start(ovr, group, case, iso, MIXED, skipping=True)
        g = _render(ovr, group)
        s = group.get_isosurface_layers()
        assert _same(g[0], whole[0]) and _same(g[1], whole[1]) and s.n == 4 and s.translucent == 1 and total(g[2]) == total(whole[2])
    finally:
        group.close()
    single.close()


@pytest.mark.parametrize("shading", (0, 2))
def test_off_restores_the_march(ovr, hip_renderer_factory, shading):
    case = _case(ovr, PC.volume("smooth", np.float32), shading=shading, rate=1.0)
    never, off = hip_renderer_factory(), hip_renderer_factory()
    hip_setup(ovr, never, case)
    _start(ovr, off, case, IC.NESTED["smooth"], THIN)
    on = _render(ovr, off)
    assert on[2].shaded_samples > 0 and off.get_isosurface_layers().translucent == 1
    off.set_isosurfaces([], [])
    off.commit()
    a, b = _render(ovr, never), _render(ovr, off)
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and not _same(on[0], b[0])
    assert [getattr(a[2], k) for k in COUNTERS] == [getattr(b[2], k) for k in COUNTERS] and a[2].pipeline == b[2].pipeline and a[2].layout == b[2].layout
    s = off.get_isosurface_layers()
    assert a[2].samples > 0 and s.n == 0 and s.translucent == 0
    never.close()
    off.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_state_intact(ovr, hip_renderer_factory):
    import ctypes as C
    import torch
    lib = ovr._lib.load()
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4 + 8 * 16, dtype=torch.float32, device=dev)
    empty = hip_renderer_factory()
    assert lib.ovr_hip_isosurface_layers_floats(empty._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 8, 0) < 0 and b"no volume" in lib.ovr_hip_last_error()
    empty.close()
    case = _case(ovr, IC.volume("ball", np.float32))
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    assert lib.ovr_hip_isosurface_layers_floats(ren._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 8, 0) < 0 and b"no isovalue" in lib.ovr_hip_last_error()
    ren.set_isosurfaces([0.5, 0.2], [0.25, 0.75])
    ren.commit()
    good = _render(ovr, ren)
    for values, bad in (([0.2, 0.5], [0.0, 0.5]), ([0.2, 0.5], [0.5, 1.0001]), ([0.2, 0.5], [np.nan, 0.5]), ([0.2, 0.5], [0.5, np.inf]), ([0.2, 0.5], [-0.5, 0.5]),
                        ([0.1, 0.2, 0.3, 0.4, 0.5], [0.5] * 5), ([np.nan], [0.5]), ([0.3, 0.3], [0.5, 0.5])):
        with pytest.raises(RuntimeError, match="ovr_hip_set_isosurface"):
            ren.set_isosurfaces(values, bad)
    v, a = (C.c_float * 2)(0.2, 0.5), (C.c_float * 2)(0.5, 0.5)
    assert lib.ovr_hip_set_isosurface_layers(ren._h, v, a, -1) < 0 and lib.ovr_hip_set_isosurface_layers(ren._h, v, a, 5) < 0 and lib.ovr_hip_set_isosurface_layers(ren._h, None, a, 2) < 0
    p = buf.data_ptr()
    for args in ((None, p, p, 1, 8, 0), (p, None, p, 1, 8, 0), (p, p, None, 1, 8, 0), (p, p, p, -1, 8, 0), (p, p, p, 1, 0, 0), (p, p, p, 1, 17, 0), (p, p, p, 1, -1, 0)):
        assert lib.ovr_hip_isosurface_layers_floats(ren._h, *args) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_isosurface_layers_floats(ren._h, p, p, p, 0, 8, 0) == 0     # n == 0: nothing to do
    assert lib.ovr_hip_isosurface_layers_floats(ren._h, p, p, p, 0, 16, 1) == 0 and lib.ovr_hip_isosurface_layers_floats(ren._h, p, p, p, 0, 1, 0) == 0
    ren.commit()
    again = _render(ovr, ren)
    s = ren.get_isosurface_layers()
    assert s.n == 2 and list(s.isovalues) == [F(0.2), F(0.5), 0.0, 0.0] and list(s.opacities) == [F(0.75), F(0.25), 0.0, 0.0] and s.translucent == 1
    assert again[2].frame_index == good[2].frame_index + 1      # nothing was queued: no reset
    assert _same(again[0], good[0]) and _same(again[1], good[1]) and again[2].samples == good[2].samples
    # opacities == NULL is ovr_hip_set_isosurfaces
    assert lib.ovr_hip_set_isosurface_layers(ren._h, v, None, 2) == 0
    ren.commit()
    s = ren.get_isosurface_layers()
    opaque = _render(ovr, ren)
    assert s.translucent == 0 and list(s.opacities) == [1.0, 1.0, 0.0, 0.0] and np.isin(opaque[0][..., 3], (0.0, 1.0)).all() and not _same(opaque[0], good[0])
    ren.close()


# ---- 7. the other known-answer entries beside committed opacities ------------------------------------------------------------------------------

def test_the_other_known_answer_entries_do_not_see_the_opacities(ovr, hip_renderer_factory):
    dims = IC.DIMS[0]
    vol = IC.volume("smooth", np.float32, dims)
    org, d, _ = PC.ray_set(dims)
    pos = (np.random.default_rng(3).random((200, 3)) * np.array(dims)).astype(F)
    case = _case(ovr, vol)
    iso = IC.NESTED["smooth"]
    opaque = _start(ovr, hip_renderer_factory(), case, iso, None)
    opaque.render()
    want_iso = [opaque.isosurface_rays(org, d, skip) for skip in (False, True)]
    want = [opaque.project_rays(org, d, mode, skip) for mode in (1, 2, 3) for skip in (False, True)]
    want_shadow = opaque.shadow_floats(pos, 0)
    assert (want_shadow > 0).any() and want_iso[0]["hit"].sum() > 20

    def check(ren, name):
        for a, b in zip([ren.isosurface_rays(org, d, skip) for skip in (False, True)], want_iso):      # the first crossing, opaque
            assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["steps"], b["steps"]) and all(_same(a[k], b[k]) for k in ("iso", "t", "normal", "shadow")), name
        for a, b in zip([ren.project_rays(org, d, mode, skip) for mode in (1, 2, 3) for skip in (False, True)], want):
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name
        assert _same(ren.shadow_floats(pos, 0), want_shadow), name

    ren = _start(ovr, hip_renderer_factory(), case, iso, THIN)
    check(ren, "committed, before a frame")
    on = _render(ovr, ren)
    assert on[2].shaded_samples > opaque.stats().shaded_samples
    check(ren, "committed, behind a translucent frame")
    s = ren.get_isosurfaces()
    assert s.n == 4 and list(s.isovalues) == [F(x) for x in iso]
    ren.close()
    opaque.close()


# ---- 8. non-finite voxels ----------------------------------------------------------------------------------------------------------------------

def test_nonfinite_voxels_follow_the_model_and_fault_nowhere(ovr, oracle, hip_renderer_factory):
    """NaN, +Inf and -Inf voxels: without skipping events, k, t*, A, steps and the shadow terms are the model's bits (a NaN sample has side 0, a NaN secant
    clamps to the interval's start); with skipping the rays and a frame complete and nothing is NaN where nothing may be"""
    I = ovr.isosurface
    dims = IC.DIMS[0]
    vol = IC.nonfinite_volume(dims)
    org, d, _ = PC.ray_set(dims)
    iso = IC.scaled(IC.NESTED["smooth"], np.float32)
    ren = _start(ovr, hip_renderer_factory(), _case(ovr, vol, rate=2.5), iso, THIN)
    clean = I.trace_rays(IC.volume("smooth", np.float32, dims), org, d, 2.5, iso, opacities=THIN)
    for rate in IC.RATES:
        ren.set_volume_sampling_rate(rate)
        ren.commit()
        want = I.trace_rays(vol, org, d, rate, iso, opacities=THIN)
        got = ren.isosurface_layer_rays(org, d, 16, False)
        assert np.array_equal(got["events"], want["n_events"]) and np.array_equal(got["steps"], want["steps"]) and np.array_equal(got["shadow_steps"], want["shadow_steps"]), rate
        assert _same(got["A"], want["A"]), rate
        f = want["flat"]
        slot = np.arange(len(f["ray"])) - np.concatenate([[0], np.cumsum(want["n_events"])[:-1]])[f["ray"]]
        keep = slot < 16
        assert np.array_equal(got["k"][f["ray"][keep], slot[keep]], f["k"][keep]) and _same(got["t"][f["ray"][keep], slot[keep]], f["t"][keep]), rate
        assert _same(got["shadow"][f["ray"][keep], slot[keep]], f["shadow"][keep]) and _same(got["A_after"][f["ray"][keep], slot[keep]], f["A"][keep]), rate
        skipped = ren.isosurface_layer_rays(org, d, 16, True)
        assert np.isfinite(skipped["t"]).all() and np.isfinite(skipped["A"]).all() and (skipped["A"] <= 1).all() and (skipped["steps"] >= 0).all()
    assert not np.array_equal(want["n_events"], clean["n_events"]) or (_bits(want["flat"]["t"]) != _bits(clean["flat"]["t"])).sum() >= 4, "the non-finite voxels touch too few rays"
    for skip in (False, True):
        ren.set_empty_space_skipping(skip)
        ren.commit()
        rgba, layer, st = _render(ovr, ren)
        assert st.rays == IC.SIZE[0] * IC.SIZE[1] and np.isin(layer[..., 2], (0.0, 1.0)).all() and np.isfinite(layer).all() and np.isfinite(rgba[..., 3]).all()
        assert st.shaded_samples > 20
        if not skip:      # the layer, the opacity and the counters are the model's; the colours are not NaN anywhere (clamp01 turns a NaN shade into 0)
            case = _case(ovr, vol, rate=IC.RATES[-1])
            ref, ref_layer, cnt = _model(ovr, oracle, case, iso, THIN, "nonfinite")
            assert _same(layer, ref_layer) and _same(rgba[..., 3], ref[..., 3]) and not np.isnan(rgba).any()
            assert st.samples == cnt["steps"] and st.shadow_samples == cnt["shadow_steps"] and st.shaded_samples == cnt["hits"]
    ren.close()


# ---- 9. the drop-in plugin ----------------------------------------------------------------------------------------------------------------------

def test_renderbatch_opacities_variable(tmp_path, ovr, oracle, hip_renderer_factory):
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
    env["OVR_HIP_ISO_OPACITIES"] = "1,0.25"
    out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / "iso")],
                         env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "[hip] isosurfaces at 0.7, 0.4 with opacities 1, 0.25" in out.stderr
    got = np.asarray(Image.open(str(tmp_path / "iso000000.png")).convert("RGBA"))
    scene, camera = ovr.vidi3d.scene_from_file(scene_path)
    ren = hip_renderer_factory()
    ren.set_fbsize((W, H))
    ren.set_frame_accumulation(True)
    ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
    ren.init(scene, camera)
    ren.set_camera(camera.eye, camera.at, camera.up)   # fovy 60 (renderer.h:149-152)
    ren.set_isosurfaces([0.7, 0.4], [1.0, 0.25])
    ren.set_empty_space_skipping(True)       # the plugin's default
    ren.commit()
    for _ in range(5 + 25):                  # main_batch.cpp:278-285: the saved frame is the mean of 30 accumulated ones
        ren.render()
    s = ren.get_isosurface_layers()
    assert ren.stats().frame_index == 30 and s.n == 2 and s.translucent == 1 and list(s.opacities)[:2] == [F(0.25), F(1.0)]
    want = np.array(ren.mapframe_rgba8(flip_vertical=True), copy=True).reshape(H, W, 4)
    assert np.array_equal(got, want) and want[..., 3].any()
    # the model's frame of the same scene: its opacity is the saved image's alpha (the PNG is flipped) - 0.25 where a ray meets the outer shell alone, once
    basis = oracle.camera_basis(camera.eye, camera.at, camera.up, 60.0, W, H).reshape(4, 3)
    model = ovr.isosurface.frame(vol, basis, (W, H), 1.0, [0.4, 0.7], np.ones((2, 3), F), (F(0.0), F(1.0)), shading=ovr.isosurface.NONE, opacities=[0.25, 1.0])
    a8 = np.asarray(oracle.rgba8(model[0], flip=True))[..., 3]      # (flipped like the PNG)
    assert np.abs(got[..., 3].astype(int) - a8.astype(int)).max() <= 1 and 100 < (model[1][..., 2] == 1).sum() < W * H - 100
    assert ((model[0][..., 3] > 0) & (model[0][..., 3] < 1)).sum() > 50
    ren.close()
