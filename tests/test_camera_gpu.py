"""The orthographic camera on the GPU (include/ovr_hip.h ovr_hip_set_camera_orthographic) against the numpy model
open-volume-renderer_amd/camera.py.  "Bits" are float32 bit patterns.  The rays, the box test, the projection and isosurface layers involve no approximated
operation: they are the model's bits.  March frames are held to the CPU oracle's trace of the model's rays by the bars tests/test_parity_gpu.py holds
perspective frames to (helpers.compare, equal sample counts), and to its bits under the exact-parity library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import camera_cases as CC
from helpers import EXACT_RUN, compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
RENDERBATCH = os.path.join(ROOT, "oracle", "_ref", "renderbatch")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
F = np.float32
TOL = 2e-4   # helpers.compare's float bar
SPECULAR = (0.3, 0.5, 0.4, 12.0)
LIGHT = (0.3, 0.8, -0.52)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, cam, size, rate=1.0, shading=0, tf="sparse", spp=1):
    colors, alphas, vr = ovr.synth.make_tfn(tf, 64, vol.dtype)
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=cam, size=size, shading=shading, rate=rate, spp=spp, convention=0, spacing=(1.0, 1.0, 1.0),
                origin=(0.0, 0.0, 0.0), fovy=60.0)


def _ortho(ovr, ren, cam, height):
    ren.set_camera(ovr.Camera(*cam, orthographic_height=height))
    ren.commit()


def _basis(ren):
    c = ren.get_camera()
    return tuple(np.array(list(v), F) for v in (c.pos, c.dir, c.hor, c.ver))


def _render(ovr, ren):
    ren.render()
    rgba, layer = hip_frame(ovr, ren)
    return rgba, layer, ren.stats()


def _noise(xy=16):
    return np.random.default_rng(18).random((xy, xy, 64), dtype=F)


# ---- 1. ovr_hip_camera_rays against the model --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", (0, 1), ids=("perspective", "orthographic"))
def test_camera_rays_vs_model(ovr, oracle, hip_renderer_factory, kind):
    K = ovr.camera
    ren = hip_renderer_factory()
    w, h = CC.BSIZE
    ren.set_fbsize((w, h))
    for cam, height in ((CC.OBLIQUE, CC.BHEIGHT), (CC.AXIS, 30.0)):
        ren.set_camera(ovr.Camera(*cam, fovy=47.0, orthographic_height=height if kind else None))
        ren.set_sample_per_pixel(1)
        ren.set_pixel_jitter(0)
        ren.commit()
        c = ren.get_camera()
        assert c.kind == kind and (c.height == F(height) and c.fovy == 0 if kind else c.fovy == F(47.0) and c.height == 0)
        basis = _basis(ren)
        model = K.basis(*cam, w, h, fovy=47.0, orthographic_height=height if kind else None)
        for got, want in zip(basis, model):      # the host's basis is the model's to rounding (the tangent is libm's there)
            assert np.abs(got - want).max() <= 8 * np.finfo(F).eps * max(np.abs(want).max(), 1.0)
        if kind:      # no tangent under this camera: the host's basis is the model's, bit for bit
            assert all(_same(got, want) for got, want in zip(basis, model))
        # pixel centres
        org, d = ren.camera_rays()
        worg, wd = K.pixel_rays(basis, w, h, None, kind)
        assert _same(org, worg) and _same(d, wd)
        if kind:
            assert _same(d, np.broadcast_to(basis[1], (h, w, 3)))
        # blue-noise jitter, two samples per pixel, the third frame
        tile = _noise()
        ren.set_noise_tile(tile)
        ren.set_pixel_jitter(1)
        ren.set_sample_per_pixel(2)
        ren.commit()
        for k in (0, 1):
            org, d = ren.camera_rays(frame_index=3, sample=k)
            xi = ovr.projection.blue_noise_variates(tile, w, h, 3, 2, k)
            worg, wd = K.pixel_rays(basis, w, h, xi, kind)
            assert _same(org, worg) and _same(d, wd), k
        # RandomTEA jitter (spp > 1, jitter mode 0) on a few pixels: RandomTEA(frame_index, pixel_index), one round per sample
        ren.set_pixel_jitter(0)
        ren.commit()
        org1, d1 = ren.camera_rays(frame_index=2, sample=1)
        for iy, ix in ((0, 0), (h - 1, w - 1), (11, 29)):
            (x0, x1), (v0, v1) = oracle.tea_floats(2, ix + iy * w)
            (x0, x1), _ = oracle.tea_floats(v0, v1)
            xi = (np.full((h, w), x0, F), np.full((h, w), x1, F))
            worg, wd = K.pixel_rays(basis, w, h, xi, kind)
            assert _same(org1[iy, ix], worg[iy, ix]) and _same(d1[iy, ix], wd[iy, ix]), (iy, ix)
    # the entry's own errors
    with pytest.raises(RuntimeError):
        ren.camera_rays(frame_index=0)
    with pytest.raises(RuntimeError):
        ren.camera_rays(sample=2)
    ren.close()


# ---- 2. the cross-section test through real frames ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (np.float32, np.uint16, np.uint8), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("am", (0, 1, 2, 3))
def test_cross_section(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    """the projections of v[z, y, x] = g[y, x] along -z at one pixel per voxel are g on the silhouette and nothing outside it.  An axis view puts exact zeros
    into every ray's direction: this is where 0 * inf in the box test would show"""
    monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
    K, P = ovr.camera, ovr.projection
    vol, g = CC.cross_section_volume(dtype), CC.cross_section().astype(F)
    # u8: g / 255 as the product samples it (one normalisation behind the filter); the exact-parity build normalises voxel by voxel
    if np.dtype(dtype) == np.uint8:
        g = (g / F(255)).astype(F) if EXACT_RUN else (g * (F(1) / F(255))).astype(F)
    ren, means = None, {}
    for (w, h), height in CC.XFRAMES:
        case = _case(ovr, vol, CC.XCAM, (w, h))
        if ren is None:
            ren = hip_setup(ovr, hip_renderer_factory(), case)
        else:
            ren.set_fbsize((w, h))
        _ortho(ovr, ren, CC.XCAM, height)
        ys, xs = CC.inner((w, h))
        want = np.zeros((h, w), bool)
        want[ys, xs] = True
        for mode in (1, 2, 3):
            ren.set_projection(mode)
            for rate in CC.XRATES:
                ren.set_volume_sampling_rate(rate)
                for skip in (False, True):
                    ren.set_empty_space_skipping(skip)
                    ren.commit()
                    rgba, layer, st = _render(ovr, ren)
                    name = (am, (w, h), mode, rate, skip)
                    assert np.array_equal(layer[..., 2] == 1, want), name
                    if mode == 3 and np.dtype(dtype) == np.uint8:
                        # the mean of n equal samples g * (1 / 255) is not that sample's bits (the sums round): the model's, with the product's 8-bit tap
                        key = ((w, h), rate)
                        if key not in means:
                            means[key] = P.frame(vol, _basis(ren), (w, h), rate, P.MEAN, np.ones((2, 3), F), np.ones(2, F), (F(0), F(1)),
                                                 sampler=None if EXACT_RUN else ovr.isosurface.product_sampler(vol), camera_kind=K.ORTHOGRAPHIC)[1]
                        assert _same(layer, means[key]) and np.abs(layer[ys, xs, 0] - g).max() <= 4 * np.finfo(F).eps * g.max(), name
                        continue
                    assert _same(layer[ys, xs, 0], g), (name, float(np.abs(layer[ys, xs, 0] - g).max()))
                    assert not rgba[~want].any() and not layer[~want].any(), name
                    assert st.rays == w * h and st.active_pixels == w * h, name
                    if not skip:
                        assert st.skipped_samples == 0, name
        # a perspective camera from the same place does not give g
        if (w, h) == CC.XFRAMES[0][0]:
            ren.set_camera(ovr.Camera(*CC.XCAM, fovy=53.13))
            ren.commit()
            assert not _same(_render(ovr, ren)[1][..., 0], g)
    ren.close()


# ---- 3. march frames against the oracle's trace of the model's rays ----------------------------------------------------------------------------

_traces = {}


def _trace(ovr, oracle, case, height):
    """the reference's march of an orthographic frame: OracleScene.trace over camera.pixel_rays (tests/test_camera_model.py licenses it), a ray that
    clipping.ignored_slab_outside flags is a miss.  Computed once per key and shared"""
    key = (np.dtype(case["vol"].dtype).name, case["cam"], case["size"], case["shading"], case["rate"], height)
    if key not in _traces:
        K = ovr.camera
        w, h = case["size"]
        sc = oracle.OracleScene(case["vol"], case["colors"], case["alphas"], case["vr"], case["cam"], w, h, fovy=case["fovy"], rate=case["rate"], shading=case["shading"])
        basis = K.basis(*case["cam"], w, h, orthographic_height=height)
        org, d = K.pixel_rays(basis, w, h, None, K.ORTHOGRAPHIC)
        nz, ny, nx = case["vol"].shape
        inv, wp = ovr.clipping.volume_constants((nx, ny, nz))
        hit = K.hits(org, d, inv, wp, kind=K.ORTHOGRAPHIC)[2].reshape(h, w)
        rgba, samples = np.zeros((h, w, 4), F), 0
        for iy in range(h):
            for ix in range(w):
                if hit[iy, ix]:
                    r, _, c = sc.trace(org[iy, ix], d[iy, ix])
                    rgba[iy, ix] = r
                    samples += c.samples
        rgba.setflags(write=False)
        _traces[key] = (rgba, samples, hit)
    return _traces[key]


MARCH_CASES = [(np.float32, "oblique", 0), (np.float32, "oblique", 1), (np.float32, "oblique", 2), (np.float32, "axis", 2), (np.float32, "axis", 0), (np.uint8, "oblique", 2),
               (np.uint16, "axis", 1)]


@pytest.mark.parametrize("dtype,cam,shading", MARCH_CASES, ids=lambda x: x if isinstance(x, str) else str(x) if isinstance(x, int) else np.dtype(x).name)
def test_march_vs_oracle_trace(ovr, oracle, hip_renderer_factory, dtype, cam, shading):
    vol = ovr.synth.make_volume(24, dtype)
    camera, height = (CC.OBLIQUE, CC.BHEIGHT) if cam == "oblique" else (CC.AXIS, 30.0)
    case = _case(ovr, vol, camera, CC.BSIZE, shading=shading)
    want, samples, hit = _trace(ovr, oracle, case, height)
    assert 100 < hit.sum() < hit.size - 100
    frames = []
    for pipeline in ((1,) if shading == 0 else (1, 2)):
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        _ortho(ovr, ren, camera, height)
        for skip in (False, True):
            ren.set_empty_space_skipping(skip)
            ren.commit()
            rgba, grad, st = _render(ovr, ren)
            name = (np.dtype(dtype).name, cam, shading, pipeline, skip)
            compare(oracle, rgba, want, name=str(name))
            assert not rgba[~hit].any() and not grad[~hit].any(), name      # the rays the miss rule drops, and the ordinary misses, are zero
            assert st.samples + st.skipped_samples == samples and st.rays == hit.size, (name, st.samples, st.skipped_samples, samples)
            assert st.pipeline == pipeline, name
            frames.append(rgba)
        ren.close()
    for f in frames[1:]:      # both pipelines, skipping on and off: one frame
        assert _same(f, frames[0])


def test_march_is_exact_under_the_exact_parity_build():
    """started the way tests/test_isosurface_gpu.py starts its child: with the exact-parity build of the kernels the march frames of an orthographic camera are
    the oracle's bits"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "march_vs_oracle_trace or (cross_section and uint8)"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == len(MARCH_CASES) + 4 and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 4. one frame, whatever the variant --------------------------------------------------------------------------------------------------------

def test_orthographic_frame_is_the_same_across_variants(ovr, hip_renderer_factory):
    """forced layouts 0 to 3, both pipelines, skipping on and off, with and without the unit clip box: one frame, bit for bit"""
    vol = ovr.synth.make_volume(24, np.float32)
    for camera, height in ((CC.AXIS, 30.0), (CC.OBLIQUE, CC.BHEIGHT)):
        case = _case(ovr, vol, camera, CC.BSIZE, shading=2)
        ref = None
        for pipeline in (1, 2):
            ren = hip_renderer_factory()
            ren.set_volume_layouts(2)      # every replica resident
            hip_setup(ovr, ren, case, pipeline=pipeline)
            _ortho(ovr, ren, camera, height)
            for layout in (0, 1, 2, 3):
                ren.set_layout_choice(layout)
                for skip in (False, True):
                    ren.set_empty_space_skipping(skip)
                    for clip in (False, True):
                        ren.set_clip_box((0.0, 0.0, 0.0), (24.0, 24.0, 24.0)) if clip else ren.set_clip_box(None)
                        ren.commit()
                        rgba, grad, st = _render(ovr, ren)
                        assert st.layout == layout and st.pipeline == pipeline
                        if ref is None:
                            ref = (rgba, grad)
                            assert rgba[..., 3].max() > 0.1
                        assert _same(rgba, ref[0]) and _same(grad, ref[1]), (pipeline, layout, skip, clip)
            ren.close()


_WHOLE_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import ovr_amd as ovr
import camera_cases as CC
from helpers import hip_frame, hip_setup
vol = ovr.synth.make_volume(24, np.float32)
colors, alphas, vr = ovr.synth.make_tfn("sparse", 64, vol.dtype)
case = dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=CC.AXIS, size=CC.BSIZE, shading=1, rate=1.0, spp=1, convention=0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=60.0)
ren = hip_setup(ovr, ovr.create_renderer("hip"), case)
ren.set_camera(ovr.Camera(*CC.AXIS, orthographic_height=30.0))
ren.commit()
ren.render()
rgba, grad = hip_frame(ovr, ren)
np.save(sys.argv[2], np.concatenate([rgba, grad], 2))
ren.close()
"""


def test_mapped_rectangle_holds_the_orthographic_frame(tmp_path, ovr, hip_renderer_factory):
    """mapframe(HOST) copies the rectangle nonzero_rect projects the box to - under this camera without the division by the distance: the cropped copy equals
    the whole one (OVR_HIP_MAP_WHOLE_FRAME, read once per process: a child)"""
    out = tmp_path / "whole.npy"
    p = subprocess.run([sys.executable, "-c", _WHOLE_CHILD, ROOT, str(out)], env=dict(os.environ, OVR_HIP_MAP_WHOLE_FRAME="1"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    whole = np.load(str(out))
    vol = ovr.synth.make_volume(24, np.float32)
    case = _case(ovr, vol, CC.AXIS, CC.BSIZE, shading=1)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _ortho(ovr, ren, CC.AXIS, 30.0)
    rgba, grad, _ = _render(ovr, ren)
    assert _same(rgba, whole[..., :4]) and _same(grad, whole[..., 4:]) and rgba[..., 3].max() > 0.1 and not rgba[0].any()
    ren.close()


def _ramp_volume():
    """v[z, y, x] = (x + 0.5) / 24: the gradient of every sample points along x, whatever the filter's rounding"""
    x = ((np.arange(24, dtype=F) + F(0.5)) / F(24)).astype(F)
    return np.ascontiguousarray(np.broadcast_to(x[None, None, :], (24, 24, 24)))


def test_cached_orthographic_frames_vs_the_lookup_model(ovr, oracle, hip_renderer_factory):
    """an orthographic frame in mode CACHED against values computed off the GPU.  Under an all-opaque transfer function every marched ray ends with its first
    sample, at p = org + tm_0 dir of the model's ray, and in a volume that is a ramp along x that sample's normal is the x axis: the pixel is
    clamp01(colour(v(p)) * lighting.shade(n, p, shadow, view = -dir)) with shadow = shadow_cache.lookup(lattice, to_object(p)) - the tap position of the
    orthographic cached twins, in place and pooled.  The lattice: the one mode CACHED built (downloaded), and a supplied random one, under which a wrong tap
    position cannot hide.  helpers.compare's bar (the normal and the shade factor use v_rsq_f32)"""
    K, P = ovr.camera, ovr.projection
    vol = _ramp_volume()
    w, h = CC.BSIZE
    case = _case(ovr, vol, CC.OBLIQUE, (w, h), shading=2, tf="opaque")
    colors = np.asarray(case["colors"], F).reshape(-1, 3)
    inv, wp = ovr.clipping.volume_constants(CC.BDIMS)
    Lu = ovr.lighting.normalize(np.asarray(LIGHT, F))
    frames = {}
    for pipeline in (1, 2):
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        ren.set_light_direction(LIGHT, 1.0)
        ren.set_material(0.2, 0.4, 0.3, 8.0)
        _ortho(ovr, ren, CC.OBLIQUE, CC.BHEIGHT)
        basis = _basis(ren)
        org, d = (a.reshape(-1, 3) for a in K.pixel_rays(basis, w, h, None, K.ORTHOGRAPHIC))
        t0, t1, hit = K.hits(org, d, inv, wp, kind=K.ORTHOGRAPHIC)
        tm, count = P.steps(t0, t1, F(1), hit)
        marched = hit & (count > 0)
        pos = ovr.lighting.fma(np.nan_to_num(tm[:, 0])[:, None], d, org)
        po = ovr.clipping.to_object(pos, inv, wp)
        rgb = P.classify(P.sample(vol, po), colors, np.ones(2, F), F(0), F(1))[:, :3]
        normal = np.broadcast_to(np.array([-1.0, 0.0, 0.0], F), pos.shape)

        def model(shadow):
            f = ovr.lighting.shade(normal, pos, shadow, Lu, basis[0], 0.2, 0.4, 0.3, 8.0, 1.0, view=K.view_vector(basis))
            out = np.zeros((w * h, 4), F)
            out[:, :3] = ovr.clipping.clamp01((rgb * f[:, None]).astype(F))
            out[:, 3] = 1
            return np.where(marched[:, None], out, F(0)).reshape(h, w, 4)

        # the model itself first, where no lattice enters: the gradient-shaded frame is shadow = 0
        ren.set_shading(1)
        ren.commit()
        got = _render(ovr, ren)
        assert got[2].pipeline == pipeline and got[2].samples == int(marched.sum()) and 100 < marched.sum() < w * h - 100
        compare(oracle, got[0], model(np.zeros(w * h, F)), name=f"gradient-shaded, pipeline {pipeline}")
        ren.set_shading(2)
        # mode CACHED: the lattice the renderer built, downloaded
        ren.set_shadow_cache(ovr.SHADOWS_CACHED, 4)
        ren.commit()
        built = _render(ovr, ren)
        lattice = ren.shadow_cache_values()
        shadow = ovr.shadow_cache.lookup(lattice, po)
        assert built[2].shadow_samples == 0 and built[2].pipeline == pipeline and ren.shadow_cache().builds == 1
        assert lattice.max() > 0.9 and lattice.min() == 0 and len(np.unique(shadow[marched])) > 20      # the first samples lie where the lattice varies
        compare(oracle, built[0], model(shadow), name=f"cached, pipeline {pipeline}")
        # a supplied random lattice of other dimensions
        sup = np.random.default_rng(24).random((6, 5, 7)).astype(F)
        ren.set_shadow_cache_values(sup)
        ren.set_shadow_cache(ovr.SHADOWS_SUPPLIED)
        ren.commit()
        supplied = _render(ovr, ren)
        want = model(ovr.shadow_cache.lookup(sup, po))
        compare(oracle, supplied[0], want, name=f"supplied, pipeline {pipeline}")
        assert np.abs(want - model(np.zeros(w * h, F))).max() > 0.05      # ... and the lattice shows in the frame
        frames[pipeline] = (built[0], supplied[0])
        ren.close()
    assert _same(frames[1][0], frames[2][0]) and _same(frames[1][1], frames[2][1])      # both pipelines: one frame


def test_shadow_cache_composition_under_the_orthographic_camera(ovr, hip_renderer_factory):
    """the cached variants' orthographic twins (tests/test_shadow_cache_gpu.py's identities): a supplied lattice of zeros is the gradient-shaded frame, of ones
    the ambient one, and a built lattice downloaded and supplied gives the built frame - bit for bit, both pipelines one frame"""
    vol = ovr.synth.make_volume(24, np.float32)
    case = _case(ovr, vol, CC.OBLIQUE, CC.BSIZE, shading=1, tf="bumps")
    frames = []
    for pipeline in (1, 2):
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        _ortho(ovr, ren, CC.OBLIQUE, CC.BHEIGHT)
        gradient = _render(ovr, ren)
        ren.set_material(0.5, 0.0, 0.0, 0.0)
        ren.commit()
        ambient = _render(ovr, ren)
        assert gradient[2].pipeline == pipeline and gradient[2].shaded_samples > 0 and not _same(gradient[0], ambient[0])
        ren.set_material()
        ren.set_shading(2)
        ren.set_shadow_cache_values(np.zeros((6, 5, 7), F))
        ren.set_shadow_cache(ovr.SHADOWS_SUPPLIED)
        ren.commit()
        zeros = _render(ovr, ren)
        assert _same(zeros[0], gradient[0]) and _same(zeros[1], gradient[1]) and zeros[2].shadow_samples == 0 and zeros[2].pipeline == pipeline
        ren.set_shadow_cache_values(np.ones((6, 5, 7), F))
        ren.commit()
        ones = _render(ovr, ren)
        assert _same(ones[0], ambient[0]) and _same(ones[1], ambient[1])
        ren.set_shadow_cache(ovr.SHADOWS_CACHED, 4)
        ren.commit()
        built = _render(ovr, ren)
        lattice = ren.shadow_cache_values()
        assert built[2].shadow_samples == 0 and not _same(built[0], zeros[0]) and not _same(built[0], ones[0])
        ren.set_shadow_cache_values(lattice)
        ren.set_shadow_cache(ovr.SHADOWS_SUPPLIED)
        ren.commit()
        again = _render(ovr, ren)
        assert _same(again[0], built[0]) and _same(again[1], built[1])
        frames.append(built[0])
        ren.close()
    assert _same(frames[0], frames[1])      # both pipelines: one frame


_JITTER_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import ovr_amd as ovr
import camera_cases as CC
from helpers import hip_frame, hip_setup
vol = CC.ball()
colors, alphas, vr = ovr.synth.make_tfn("sparse", 64, vol.dtype)
case = dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=CC.OBLIQUE, size=(136, 88), shading=0, rate=1.0, spp=2, convention=0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=60.0)
out = []
for height in (120.0, 36.0, 9.0):
    ren = hip_setup(ovr, ovr.create_renderer("hip"), case)
    ren.set_camera(ovr.Camera(*CC.OBLIQUE, orthographic_height=height))
    ren.set_projection(1)
    ren.commit()
    ren.render()
    rgba, grad = hip_frame(ovr, ren)
    st = ren.stats()
    out.append(np.concatenate([rgba, grad], 2))
    out.append(np.full_like(out[-1], float(st.samples)))
    ren.close()
np.save(sys.argv[2], np.stack(out))
"""


def test_jittered_orthographic_frames_launch_what_they_need(tmp_path, ovr, hip_renderer_factory):
    """several samples per pixel or jittered ones: the schedule culls a block whose pixel rectangle, widened by 1.5 pixels, lies apart from the rectangle the
    box projects to along the parallel rays.  No ray that hits may be culled: the blue-noise frames are the model's, bit for bit, and the RandomTEA frames
    (which the model does not restate) equal a process that launches every block (OVR_HIP_EMPTY_BLOCKS=0, read once per process: two children)"""
    K, P = ovr.camera, ovr.projection
    vol = CC.ball()
    w, h = 136, 88
    case = _case(ovr, vol, CC.OBLIQUE, (w, h), spp=2)
    tile = _noise()
    colors, alphas = np.asarray(case["colors"], F).reshape(-1, 3), np.asarray(case["alphas"], F).reshape(-1, 2)[:, 1]
    for height in (120.0, 36.0, 9.0):      # the box small in the frame, filling it, and larger than it
        ren = hip_renderer_factory()
        ren.set_noise_tile(tile)
        ren.set_pixel_jitter(1)
        hip_setup(ovr, ren, case)
        _ortho(ovr, ren, CC.OBLIQUE, height)
        ren.set_projection(P.MAXIMUM)
        ren.commit()
        got = _render(ovr, ren)
        want = P.frame(vol, _basis(ren), (w, h), 1.0, P.MAXIMUM, colors, alphas, P.normalized_range(case["vr"], vol.dtype), spp=2, noise=tile, camera_kind=K.ORTHOGRAPHIC)
        assert _same(got[1], want[1]) and _same(got[0], want[0]), height
        assert got[2].samples == want[2]["steps"] and got[2].rays == 2 * w * h and got[2].active_pixels == w * h
        assert height != 120.0 or (got[1][..., 2] == 0).mean() > 0.8
        ren.close()
    outs = []
    for tag, extra in (("culled", {}), ("every", {"OVR_HIP_EMPTY_BLOCKS": "0"})):
        env = dict(os.environ, **extra)
        if not extra:
            env.pop("OVR_HIP_EMPTY_BLOCKS", None)
        path = tmp_path / f"{tag}.npy"
        p = subprocess.run([sys.executable, "-c", _JITTER_CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs.append(np.load(str(path)))
    assert _same(outs[0], outs[1]) and outs[0][0][..., 3].max() > 0 and outs[0][1].max() > 0


def test_clipped_orthographic_projection_vs_model(ovr, hip_renderer_factory):
    """a real clip box under the orthographic camera: the model's layer, bit for bit"""
    K, P = ovr.camera, ovr.projection
    vol = CC.ball()
    w, h = CC.BSIZE
    case = _case(ovr, vol, CC.OBLIQUE, (w, h))
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _ortho(ovr, ren, CC.OBLIQUE, CC.BHEIGHT)
    lower, upper = (5.0, -np.inf, 3.5), (19.0, 14.25, np.inf)
    ren.set_clip_box(lower, upper)
    ren.set_projection(P.MAXIMUM)
    ren.commit()
    rgba, layer, st = _render(ovr, ren)
    inv, wp = ovr.clipping.volume_constants(CC.BDIMS)
    colors, alphas = np.asarray(case["colors"], F).reshape(-1, 3), np.asarray(case["alphas"], F).reshape(-1, 2)[:, 1]
    want = P.frame(vol, _basis(ren), (w, h), 1.0, P.MAXIMUM, colors, alphas, P.normalized_range(case["vr"], vol.dtype), clip=ovr.clipping.object_box(lower, upper, inv, wp),
                   camera_kind=K.ORTHOGRAPHIC)
    assert _same(layer, want[1]) and _same(rgba, want[0]) and 50 < (layer[..., 2] == 1).sum() < w * h - 50
    assert st.samples == want[2]["steps"]
    ren.close()


# ---- 5. projection and isosurface frames against their models ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", ("oblique", "axis"))
def test_projection_and_isosurface_frames_vs_model(ovr, oracle, hip_renderer_factory, cam):
    K, P, I = ovr.camera, ovr.projection, ovr.isosurface
    vol = CC.ball()
    w, h = CC.BSIZE
    camera, height = (CC.OBLIQUE, CC.BHEIGHT) if cam == "oblique" else (CC.AXIS, 30.0)
    case = _case(ovr, vol, camera, (w, h), shading=2)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    _ortho(ovr, ren, camera, height)
    basis = _basis(ren)
    colors, alphas = np.asarray(case["colors"], F).reshape(-1, 3), np.asarray(case["alphas"], F).reshape(-1, 2)[:, 1]
    tf_range = P.normalized_range(case["vr"], vol.dtype)
    for mode in (P.MAXIMUM, P.MINIMUM, P.MEAN):
        for skip in (False, True):
            ren.set_projection(mode)
            ren.set_empty_space_skipping(skip)
            ren.commit()
            rgba, layer, st = _render(ovr, ren)
            want = P.frame(vol, basis, (w, h), 1.0, mode, colors, alphas, tf_range, skipping=skip, camera_kind=K.ORTHOGRAPHIC)
            assert _same(layer, want[1]) and _same(rgba, want[0]), (cam, mode, skip)
            assert st.samples + st.skipped_samples == want[2]["steps"] and st.samples == want[2]["fetched"] and st.rays == w * h
            assert 100 < (layer[..., 2] == 1).sum() < w * h - 100
    ren.set_projection(P.OFF)
    ren.set_empty_space_skipping(False)
    ren.set_light_direction(LIGHT, 1.0)
    ren.set_material(*SPECULAR)         # the specular term: V = -dir for every sample
    for shading in (2, 1, 0):
        ren.set_shading(shading)
        ren.set_isosurfaces([0.35, 0.6])
        ren.commit()
        rgba, layer, st = _render(ovr, ren)
        want = I.frame(vol, basis, (w, h), 1.0, [0.35, 0.6], colors, tf_range, shading=shading, light=LIGHT, material=SPECULAR, camera_kind=K.ORTHOGRAPHIC)
        assert _same(layer, want[1]), (cam, shading)
        if EXACT_RUN or shading == 0:
            assert _same(rgba, want[0]), (cam, shading)
        else:
            compare(oracle, rgba, want[0], name=str((cam, shading)))
        assert st.shaded_samples == want[2]["hits"] and want[2]["hits"] > 100
        if shading == 1:     # ... and the view vector is -dir: a normal along the orthographic half vector, at a position off to the side of the view
            Lu = ovr.lighting.normalize(np.asarray(LIGHT, F))
            nrm = ovr.lighting.normalize((Lu + K.view_vector(basis)).astype(F))[None, :]
            pos = (basis[0] + F(30) * basis[1] + F(0.4) * basis[2]).astype(F)[None, :]
            persp = ovr.lighting.shade(nrm, pos, np.zeros(1, F), Lu, basis[0], *SPECULAR)
            orth = ovr.lighting.shade(nrm, pos, np.zeros(1, F), Lu, basis[0], *SPECULAR, view=K.view_vector(basis))
            got = ren.shade_floats(nrm, pos, np.zeros(1, F))
            assert abs(float(got[0]) - float(orth[0])) <= TOL and abs(float(persp[0]) - float(orth[0])) > 10 * TOL, (got, orth, persp)
    ren.close()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------------------------

def test_camera_state(ovr, hip_renderer_factory):
    vol = CC.ball()
    case = _case(ovr, vol, CC.OBLIQUE, CC.BSIZE, shading=1)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    first = _render(ovr, ren)
    assert ren.get_camera().kind == 0
    # the queued camera is not the committed one
    ren.set_camera(ovr.Camera(*CC.OBLIQUE, orthographic_height=CC.BHEIGHT))
    assert ren.get_camera().kind == 0
    ren.commit()
    c = ren.get_camera()
    assert c.kind == 1 and c.height == F(CC.BHEIGHT) and tuple(c.eye) == tuple(F(x) for x in CC.OBLIQUE[0])
    a = _render(ovr, ren)
    assert a[2].frame_index == 1 and not _same(a[0], first[0])
    b = _render(ovr, ren)
    assert b[2].frame_index == 2
    # a changed height resets the accumulation
    ren.set_camera(ovr.Camera(*CC.OBLIQUE, orthographic_height=CC.BHEIGHT * 0.5))
    ren.commit()
    z = _render(ovr, ren)
    assert z[2].frame_index == 1 and not _same(z[0], a[0])
    # EINVAL leaves the state unchanged
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            ren.set_camera(ovr.Camera(*CC.OBLIQUE, orthographic_height=bad))
    ren.commit()
    assert ren.get_camera().height == F(CC.BHEIGHT * 0.5) and _render(ovr, ren)[2].frame_index == 2
    # back to the first orthographic camera, then to the perspective one: the first frames' bits
    ren.set_camera(ovr.Camera(*CC.OBLIQUE, orthographic_height=CC.BHEIGHT))
    ren.commit()
    assert _same(_render(ovr, ren)[0], a[0])
    ren.set_camera(ovr.Camera(*CC.OBLIQUE, fovy=case["fovy"]))
    ren.commit()
    again = _render(ovr, ren)
    assert ren.get_camera().kind == 0 and _same(again[0], first[0]) and _same(again[1], first[1]) and again[2].samples == first[2].samples
    ren.close()


def test_device_group_and_image_shards(ovr, hip_renderer_factory):
    """a device group of two members on one card, and an image shard pair, give the single renderer's orthographic frame"""
    vol = ovr.synth.make_volume(24, np.float32)
    case = _case(ovr, vol, CC.AXIS, CC.BSIZE, shading=2)
    single = hip_setup(ovr, hip_renderer_factory(), case)
    _ortho(ovr, single, CC.AXIS, 30.0)
    want = _render(ovr, single)
    single.close()
    group = ovr.create_renderer("hip", devices=[0, 0])
    try:
        hip_setup(ovr, group, case)
        _ortho(ovr, group, CC.AXIS, 30.0)
        got = _render(ovr, group)
        assert group.get_camera().kind == 1 and _same(got[0], want[0]) and _same(got[1], want[1])
    finally:
        group.close()
    merged = np.zeros_like(want[0])
    for rank in (0, 1):
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        ren.set_image_shard(rank, 2, 8, 8)
        _ortho(ovr, ren, CC.AXIS, 30.0)
        rgba = _render(ovr, ren)[0]
        iy, ix = np.mgrid[0:CC.BSIZE[1], 0:CC.BSIZE[0]]
        own = ((ix // 8 + iy // 8) % 2) == rank
        merged[own] = rgba[own]
        ren.close()
    assert _same(merged, want[0])


# ---- 7. the drop-in plugin ---------------------------------------------------------------------------------------------------------------------

def test_renderbatch_orthographic_variable(tmp_path, ovr, oracle, hip_renderer_factory):
    """OVR_HIP_ORTHOGRAPHIC through the unmodified batch app against the Python renderer's rgba8, by the bar tests/test_clipping_gpu.py holds the batch app's
    march frames to: <= 1 on every 8-bit channel (the reference rasterises the colour control points itself, the last ulp of the table differs)"""
    if not (os.path.exists(RENDERBATCH) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/renderbatch or plugin/libdevice_hip.so missing: they are built by __graft_entry__.build() where the reference tree is present and travel with the snapshot")
    from PIL import Image
    n, W, H = 40, 96, 64
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("bumps", 256, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.25,
                                        projection_mode="ORTHOGRAPHIC")
    env0 = dict(os.environ)
    env0["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env0.get("LD_LIBRARY_PATH", "")])
    for k in ("OVR_HIP_ORTHOGRAPHIC", "OVR_HIP_QUIET"):
        env0.pop(k, None)

    def batch(tag, **extra):
        out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / tag)],
                             env=dict(env0, **extra), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        return np.asarray(Image.open(str(tmp_path / f"{tag}000000.png")).convert("RGBA")), out.stderr

    plain, err = batch("plain")       # the reference's loader never sets the camera's type: the file's projectionMode does not reach the device
    assert "[hip] orthographic camera" not in err
    got, err = batch("ortho", OVR_HIP_ORTHOGRAPHIC="56.5")
    assert "[hip] orthographic camera: image height 56.5" in err
    auto, err = batch("auto", OVR_HIP_ORTHOGRAPHIC="auto")
    assert "(auto)" in err
    scene, camera = ovr.vidi3d.scene_from_file(scene_path)
    assert camera.orthographic_height is not None and abs(camera.orthographic_height - ovr.camera.auto_height(camera.eye, camera.at, 45.0)) < 1e-9

    def host(height):
        ren = hip_renderer_factory()
        ren.set_fbsize((W, H))
        ren.set_frame_accumulation(True)
        ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
        ren.init(scene, camera)
        ren.set_camera(ovr.Camera(camera.eye, camera.at, camera.up, orthographic_height=height))
        ren.commit()
        ren.render()
        assert ren.get_camera().kind == 1
        return oracle.rgba8(hip_frame(ovr, ren)[0], flip=True).reshape(H, W, 4)

    want = host(56.5)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1 and want[..., 3].any() and not want[..., 3].all()
    # auto: 2 |from - at| tan(fovy / 2) with the fovy the app passes on - 60 degrees, whatever the file says (renderer.h:149-152)
    want_auto = host(ovr.camera.auto_height(camera.eye, camera.at, 60.0))
    assert np.abs(auto.astype(int) - want_auto.astype(int)).max() <= 1
    assert np.abs(got.astype(int) - plain.astype(int)).max() > 20
