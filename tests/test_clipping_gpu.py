"""The clip box on the GPU (include/ovr_hip.h ovr_hip_set_clip_box).

The oracle pin is "clip = crop": the UNMODIFIED CPU oracle renders the cropped volume V[lo:hi] at grid_origin = lo, the renderer renders V under the world
clip box lo .. hi.  The layers just outside the cut are overwritten with the layers just inside it first, so that the cropped volume's clamp-to-edge taps read
what the clipped march's taps read in V; the cut faces lie at multiples of 4 of a 32^3 (64^3) volume and the camera coordinates are dyadic, so every
object-space coordinate is exact in both set-ups and the two marches are the same floats: under the exact-parity build frame, gradient layer and counters are
EQUAL (test_clipping_is_exact_under_the_exact_parity_build starts this file that way), in the product they meet the parity suites' bars.

Shaded cuts with an upper face inside the volume are NOT an identity - the cropped volume's gradient flips to a backward difference in its last layer (measured
0.29-0.49 on these inputs) - and are not tested against a crop: upper faces under shading are covered by the unshaded cuts, the interval hook (bit for bit
against clipping.py) and the invariants."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import EXACT_RUN, compare, hip_frame, hip_setup, make_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
RENDERBATCH = os.path.join(ROOT, "oracle", "_ref", "renderbatch")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
F = np.float32
INF = float("inf")
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")

CAMERAS = {  # eye, at; up +y, fovy 40
    "cut": ((-30.5, 28.25, -44.0), (20.0, 16.0, 20.0)),
    "back": ((70.0, 40.25, 66.5), (20.0, 16.0, 22.0)),
    "inside": ((24.5, 17.25, 21.0), (10.0, 15.0, 0.0)),
    "axis": ((24.0, 16.0, -50.0), (24.0, 16.0, 0.0)),
}
CONFIGS = [("sparse", "cut", 1.0, 2), ("dense", "cut", 2.0, 2), ("bumps", "back", 1.0, 2), ("dense", "inside", 3.0, 2), ("sparse", "axis", 1.0, 1),
           ("dense", "back", 0.5, 0)]
DTYPES = [np.float32, np.uint16, np.uint8]
SIZE = (48, 40)


def _counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


_volumes = {}


def cut_volume(ovr, n, dtype, lo, hi):
    """V of n^3 voxels with the layers just outside the cut [lo, hi) overwritten by the layers just inside (shared, read-only), and its crop"""
    key = (n, np.dtype(dtype).name, tuple(lo), tuple(hi))
    if key not in _volumes:
        v = ovr.synth.make_volume(n, dtype).copy()
        for k in range(3):   # volume axes are (z, y, x)
            ax = 2 - k
            idx = [slice(None)] * 3
            src = [slice(None)] * 3
            if lo[k] > 0:
                idx[ax], src[ax] = lo[k] - 1, lo[k]
                v[tuple(idx)] = v[tuple(src)]
            if hi[k] < n:
                idx[ax], src[ax] = hi[k], hi[k] - 1
                v[tuple(idx)] = v[tuple(src)]
        v.setflags(write=False)
        crop = np.ascontiguousarray(v[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])
        crop.setflags(write=False)
        _volumes[key] = (v, crop)
    return _volumes[key]


def crop_case(ovr, n, dtype, lo, hi, tf, cam, rate, shading, size=SIZE, spp=1, scale=1.0):
    vol, crop = cut_volume(ovr, n, dtype, lo, hi)
    colors, alphas, vr = ovr.synth.make_tfn(tf, 256, dtype)
    eye, at = CAMERAS[cam]
    camera = (tuple(scale * x for x in eye), tuple(scale * x for x in at), (0.0, 1.0, 0.0))
    case = dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=camera, size=size, shading=shading, rate=rate, spp=spp, convention=0, spacing=(1.0, 1.0, 1.0),
                origin=(0.0, 0.0, 0.0), fovy=40.0)
    return case, crop


def oracle_crop(oracle, case, crop, lo, **kw):
    w, h = case["size"]
    return oracle.OracleScene(crop, case["colors"], case["alphas"], case["vr"], case["cam"], w, h, fovy=case["fovy"], spp=case["spp"], rate=case["rate"],
                              shading=case["shading"], grid_origin=tuple(float(x) for x in lo), grid_spacing=(1, 1, 1), **kw)


def check_against_crop(oracle, name, rgba, grad, st, ref, ref_grad, cnt, exact_capable=True):
    df = float(np.abs(rgba - ref).max())
    print(f"{name}: max float difference {df:.3g}; samples {st.samples} / {cnt.samples}, shaded {st.shaded_samples} / {cnt.shaded_samples} (borderline {cnt.borderline_samples}), "
          f"shadow {st.shadow_samples} / {cnt.shadow_samples_visible}")
    assert np.isfinite(ref).all()
    if exact_capable:
        compare(oracle, rgba, ref, name=name)     # the exact-parity run: equality of every float
    else:                                         # helpers.compare's product bar, spelled out (see case 3)
        assert not np.isnan(rgba).any() and df <= 2e-4 and np.abs(oracle.rgba8(rgba).astype(int) - oracle.rgba8(ref).astype(int)).max() <= 1, (name, df)
    assert st.rays == cnt.rays
    assert st.samples == cnt.samples, (name, "primary sample count differs from the oracle's")
    if EXACT_RUN and exact_capable:
        assert _bits_equal(grad, ref_grad), name
        assert st.shaded_samples == cnt.shaded_samples and st.shadow_samples == cnt.shadow_samples_visible, name
    else:
        assert abs(int(st.shaded_samples) - int(cnt.shaded_samples)) <= int(cnt.borderline_samples), name


def render_clipped(ovr, ren, case, lo, hi, accumulate=False, pipeline=0, frames=1):
    hip_setup(ovr, ren, case, accumulate=accumulate, pipeline=pipeline)
    ren.set_clip_box(lo, hi)
    ren.commit()
    for _ in range(frames):
        ren.render()
    return hip_frame(ovr, ren) + (ren.stats(),)


# ---- 1. shaded, lower-corner cube cut: clip = crop ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("config", range(len(CONFIGS)), ids=lambda i: "-".join(map(str, CONFIGS[i])))
def test_corner_cut_vs_oracle_crop(ovr, oracle, hip_renderer_factory, config, dtype):
    """the literal light runs towards -x, +y, -z: shadow rays leave the cut through two of its faces - an unclipped shadow march fails this"""
    tf, cam, rate, shading = CONFIGS[config]
    lo, hi = (16, 16, 16), (32, 32, 32)
    case, crop = crop_case(ovr, 32, dtype, lo, hi, tf, cam, rate, shading)
    ref, ref_grad, cnt = oracle_crop(oracle, case, crop, lo).render()
    assert cnt.samples > 0 and (shading == 0 or cnt.shaded_samples > 0)
    for pipeline in (1, 2) if shading else (1,):
        ren = hip_renderer_factory()
        rgba, grad, st = render_clipped(ovr, ren, case, lo, hi, pipeline=pipeline)
        assert st.pipeline == pipeline
        ren.close()
        check_against_crop(oracle, f"{CONFIGS[config]} {np.dtype(dtype).name} pipeline {pipeline}", rgba, grad, st, ref, ref_grad, cnt)


def test_corner_cut_vs_oracle_crop_64(ovr, oracle, hip_renderer_factory):
    lo, hi = (32, 32, 32), (64, 64, 64)
    case, crop = crop_case(ovr, 64, np.float32, lo, hi, "sparse", "cut", 1.0, 2, scale=2.0)
    ref, ref_grad, cnt = oracle_crop(oracle, case, crop, lo).render()
    ren = hip_renderer_factory()
    rgba, grad, st = render_clipped(ovr, ren, case, lo, hi)
    ren.close()
    assert cnt.shadow_samples_visible > 0
    check_against_crop(oracle, "64^3 corner cut", rgba, grad, st, ref, ref_grad, cnt)


def test_corner_cut_vs_oracle_crop_spp3_accumulated(ovr, oracle, hip_renderer_factory):
    lo, hi = (16, 16, 16), (32, 32, 32)
    case, crop = crop_case(ovr, 32, np.uint16, lo, hi, "bumps", "back", 1.0, 2, spp=3)
    ref, ref_grad, cnt = oracle_crop(oracle, case, crop, lo).render(frames=2, accumulate=True)
    for pipeline in (1, 2):
        ren = hip_renderer_factory()
        rgba, grad, st = render_clipped(ovr, ren, case, lo, hi, accumulate=True, pipeline=pipeline, frames=2)
        assert st.frame_index == 2
        ren.close()
        check_against_crop(oracle, f"spp 3, two frames, pipeline {pipeline}", rgba, grad, st, ref, ref_grad, cnt)


def test_corner_cut_vs_oracle_crop_odd_size(ovr, oracle, hip_renderer_factory):
    lo, hi = (16, 16, 16), (32, 32, 32)
    case, crop = crop_case(ovr, 32, np.float32, lo, hi, "dense", "cut", 2.0, 2, size=(50, 37))
    ref, ref_grad, cnt = oracle_crop(oracle, case, crop, lo).render()
    ren = hip_renderer_factory()
    rgba, grad, st = render_clipped(ovr, ren, case, lo, hi)
    ren.close()
    check_against_crop(oracle, "50 x 37", rgba, grad, st, ref, ref_grad, cnt)


def test_sparse_sampled_pixels_equal_the_dense_clipped_frame(ovr, oracle, hip_renderer_factory):
    lo, hi = (16, 16, 16), (32, 32, 32)
    case, _ = crop_case(ovr, 32, np.float32, lo, hi, "sparse", "cut", 1.0, 2)
    noise = (np.random.default_rng(11).integers(0, 256, size=(32, 32, 64)) / 255.0).astype(F)
    focus = ((0.5, 0.5), 0.4, 0.1)
    dense = hip_renderer_factory()
    want, want_grad, _ = render_clipped(ovr, dense, case, lo, hi)
    dense.close()
    for pipeline in (1, 2):
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        ren.set_noise_tile(noise)
        ren.set_focus(*focus)
        ren.set_sparse_sampling(True)
        ren.set_clip_box(lo, hi)
        ren.commit()
        ren.render()
        got, got_grad = hip_frame(ovr, ren)
        st = ren.stats()
        ren.close()
        xy = oracle.sparse_mask(1, SIZE[0], SIZE[1], *focus, noise).reshape(-1, 2)
        assert 50 < len(xy) < SIZE[0] * SIZE[1] and st.active_pixels == len(xy)
        assert _bits_equal(got[xy[:, 1], xy[:, 0]], want[xy[:, 1], xy[:, 0]]) and _bits_equal(got_grad[xy[:, 1], xy[:, 0]], want_grad[xy[:, 1], xy[:, 0]])
        assert want[xy[:, 1], xy[:, 0], 3].max() > 0


# ---- 2. SHADE_NONE, any half cut ------------------------------------------------------------------------------------------------------------------

HALF_CUTS = [((0, 0, 0), (16, 16, 16)), ((8, 8, 8), (24, 24, 24)), ((4, 4, 4), (20, 20, 20)), ((0, 16, 0), (32, 32, 16)), ((8, 0, 16), (24, 32, 32))]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("cut", range(len(HALF_CUTS)), ids=lambda i: "%s..%s" % HALF_CUTS[i])
def test_unshaded_half_cut_vs_oracle_crop(ovr, oracle, hip_renderer_factory, cut, dtype):
    lo, hi = HALF_CUTS[cut]
    hit_any = 0
    for cam in CAMERAS:
        case, crop = crop_case(ovr, 32, dtype, lo, hi, "dense", cam, 1.0, 0)
        ref, ref_grad, cnt = oracle_crop(oracle, case, crop, lo).render()
        ren = hip_renderer_factory()
        rgba, grad, st = render_clipped(ovr, ren, case, lo, hi)
        ren.close()
        check_against_crop(oracle, f"unshaded {lo}..{hi} {cam} {np.dtype(dtype).name}", rgba, grad, st, ref, ref_grad, cnt)
        hit_any += int(cnt.samples > 0)
    assert hit_any >= 3


# ---- 3. shaded, non-cubic lower cuts of 64 (product bar: not bit-identical even between two CPU restatements - the normal is normalised before an
#         anisotropic scale; measured <= 1.8e-7 on RGBA with all counters equal) -------------------------------------------------------------------

@pytest.mark.parametrize("lo", [(16, 0, 16), (0, 0, 16), (32, 0, 0)], ids=str)
def test_non_cubic_lower_cut_vs_oracle_crop(ovr, oracle, hip_renderer_factory, lo):
    hi = (64, 64, 64)
    case, crop = crop_case(ovr, 64, np.float32, lo, hi, "sparse", "cut", 1.0, 2, scale=2.0)
    ref, ref_grad, cnt = oracle_crop(oracle, case, crop, lo).render()
    ren = hip_renderer_factory()
    rgba, grad, st = render_clipped(ovr, ren, case, lo, hi)
    ren.close()
    assert cnt.shaded_samples > 0
    check_against_crop(oracle, f"non-cubic {lo}", rgba, grad, st, ref, ref_grad, cnt, exact_capable=False)


def test_clipping_is_exact_under_the_exact_parity_build():
    """started the way tests/test_parity_exact_gpu.py starts its children: the exact-parity build of the kernels, the oracle in its "det" mode, helpers.compare =
    equality of every float.  Cases 1 and 2 - frame, gradient layer and every counter, the shadow count included - and the interval hook: bit for bit."""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "corner_cut or half_cut or hook"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) >= 18 + 3 + 15 + 1 and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 4. the interval hook against clipping.py, bit for bit ---------------------------------------------------------------------------------------

def _rays(rng, n, dims, spacing, origin):
    ext = np.array(dims, np.float64) * np.array(spacing, np.float64)
    org = (np.array(origin) + (rng.random((n, 3)) * 3.0 - 1.0) * ext).astype(F)              # inside and outside the volume
    d = rng.standard_normal((n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    k = n // 10
    d[:k, rng.integers(0, 3, k)] = 0.0                                                         # axis-parallel: the ignored slab
    d[k:2 * k, 0] = F(1e-39)                                                                   # below FLT_MIN after the scale
    d[2 * k:3 * k, 1] = F(-3e-37)                                                              # just above / below it, depending on inv_scale
    d[3 * k:4 * k, 2] = F(1.2e-38) * np.array(dims[2] * spacing[2], F)                         # around FLT_MIN itself
    org[4 * k:5 * k] = (np.array(origin) + rng.random((k, 3)) * ext).astype(F)                 # inside the volume
    return org, d.astype(F)


@pytest.mark.parametrize("volume", [dict(dims=(32, 32, 32), spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)),
                                    dict(dims=(40, 23, 31), spacing=(1.0, 1.5, 0.75), origin=(3.0, -2.0, 5.0))], ids=["cube", "aniso"])
def test_interval_hook_vs_model(ovr, oracle, hip_renderer_factory, volume):
    clipping = ovr.clipping
    dims, spacing, origin = volume["dims"], volume["spacing"], volume["origin"]
    case = make_case(ovr, oracle, n=0, dims=dims, spacing=spacing, origin=origin, tf="dense", cam="oblique", size=(32, 24), shading=0)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    inv, wp = clipping.volume_constants(dims, spacing, origin)
    ext = [d * s for d, s in zip(dims, spacing)]
    top = [o + e for o, e in zip(origin, ext)]
    boxes = [None,
             ((origin[0] + 5.5, -INF, origin[2] + 9.0), (origin[0] + 27.0, origin[1] + 20.25, INF)),
             (tuple(origin), tuple(o + e / 2 for o, e in zip(origin, ext))),                     # touching the volume's lower faces
             (tuple(o + e / 4 for o, e in zip(origin, ext)), tuple(top)),                         # ... and its upper faces
             (tuple(o - 1.0 for o in origin), tuple(t + 1.0 for t in top)),                       # containing it
             ((origin[0] + 3.0, origin[1], origin[2]), (origin[0] + 3.0, top[1], top[2])),        # flat: empty
             (tuple(t + 1.0 for t in top), tuple(t + 2.0 for t in top))]                          # beside it: empty
    rng = np.random.default_rng(5)
    for i, box in enumerate(boxes):
        if box is None:
            ren.set_clip_box(None)
            lo, hi = np.zeros(3, F), np.ones(3, F)
        else:
            ren.set_clip_box(*box)
            lo, hi = clipping.object_box(box[0], box[1], inv, wp)
        ren.commit()
        cb = ren.clip_box()
        assert cb.enabled == (box is not None)
        assert _bits_equal(np.array(list(cb.object_lower), F), lo) and _bits_equal(np.array(list(cb.object_upper), F), hi), (i, list(cb.object_lower), lo)
        org, d = _rays(rng, 3000, dims, spacing, origin)
        t0, t1, hit = ren.clip_intervals(org, d)
        w0, w1, whit = clipping.world_intervals(org, d, inv, wp, lo, hi)
        assert np.array_equal(hit, whit), (i, int((hit != whit).sum()))
        assert _bits_equal(t0, w0) and _bits_equal(t1, w1), (i, int((t0.view(np.uint32) != w0.view(np.uint32)).sum()), int((t1.view(np.uint32) != w1.view(np.uint32)).sum()))
        if i in (5, 6):
            assert not hit.any()
        elif i != 6:
            assert 100 < hit.sum() < len(hit)
    ren.close()


# ---- 5. invariants under one non-trivial clip box -------------------------------------------------------------------------------------------------

BOX = ((5.5, -INF, 9.0), (27.0, 20.25, INF))


def _inv_case(ovr, oracle, **kw):
    args = dict(n=32, tf="bumps", cam="oblique", size=(96, 64), shading=2)
    args.update(kw)
    return make_case(ovr, oracle, **args)


def _clipped(ovr, ren, case, box=BOX, **setup):
    hip_setup(ovr, ren, case, **setup)
    ren.set_clip_box(*box)
    return ren


def _same(frames):
    base = next(iter(frames.values()))
    for k, (rgba, grad, cnt) in frames.items():
        assert _bits_equal(rgba, base[0]) and _bits_equal(grad, base[1]), k
        assert cnt == base[2], (k, cnt, base[2])
    return base


def test_invariant_pipelines_skipping_layouts(ovr, oracle, hip_renderer_factory):
    case = _inv_case(ovr, oracle)
    frames = {}
    for pipeline in (1, 2):
        for skip in (False, True):
            for layout in (0, 1, 2, 3):
                if layout and (pipeline, skip) not in ((1, False), (2, True)):
                    continue
                ren = hip_renderer_factory()
                ren.set_volume_layouts(2)
                ren.set_layout_choice(layout)
                _clipped(ovr, ren, case, pipeline=pipeline)
                ren.set_empty_space_skipping(skip)
                ren.commit()
                ren.render()
                st = ren.stats()
                assert st.layout == layout and st.pipeline == pipeline
                frames[(pipeline, skip, layout)] = hip_frame(ovr, ren) + ((st.rays, st.samples + st.skipped_samples, st.shaded_samples, st.shadow_samples + st.skipped_shadow_samples),)
                ren.close()
    base = _same(frames)
    # ... and it is not the unclipped frame: fewer samples, another picture
    ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=1)
    ren.render()
    st = ren.stats()
    assert st.samples > base[2][1] > 0 and np.abs(hip_frame(ovr, ren)[0] - base[0]).max() > 0.05
    ren.close()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_invariant_addressing_modes(ovr, oracle, hip_renderer_factory, monkeypatch, dtype):
    case = _inv_case(ovr, oracle, size=(72, 56), dtype=dtype)
    frames = []
    for am in (0, 1, 2, 3):
        monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
        for pipeline in (2, 1):
            ren = _clipped(ovr, hip_renderer_factory(), case, pipeline=pipeline)
            ren.commit()
            ren.render()
            frames.append(hip_frame(ovr, ren)[0].copy())
            ren.close()
    for f in frames[1:]:
        assert _bits_equal(f, frames[0])
    assert frames[0][..., 3].max() > 0


def test_invariant_shade_order_and_lds_staging(ovr, oracle, hip_renderer_factory, monkeypatch):
    case = _inv_case(ovr, oracle, tf="dense", size=(128, 96))
    frames = {}
    for order in ("0", None):
        if order is None:
            monkeypatch.delenv("OVR_HIP_SHADE_ORDER", raising=False)
        else:
            monkeypatch.setenv("OVR_HIP_SHADE_ORDER", order)   # read when the renderer is created
        ren = _clipped(ovr, hip_renderer_factory(), case, pipeline=2)
        ren.commit()
        ren.render()
        st = ren.stats()
        assert st.pipeline == 2
        frames[("order", order)] = hip_frame(ovr, ren) + (_counters(st),)
        ren.close()
    ren = _clipped(ovr, hip_renderer_factory(), case, pipeline=2)
    ren.set_lds_staging(True)
    ren.commit()
    ren.render()
    frames["lds requested"] = hip_frame(ovr, ren) + (_counters(ren.stats()),)
    ren.close()
    _same(frames)
    # the march LDS staging exists for (unshaded, f32, in place): a clipped frame takes the ordinary march - the same frame, lds_rounds == 0
    plain = dict(case, shading=0)
    got = {}
    for staging in (False, True):
        ren = _clipped(ovr, hip_renderer_factory(), plain)
        ren.set_lds_staging(staging)
        ren.commit()
        ren.render()
        st = ren.stats()
        assert st.lds_rounds == 0
        got[staging] = hip_frame(ovr, ren) + (_counters(st),)
        ren.close()
    _same(got)
    ren = hip_setup(ovr, hip_renderer_factory(), plain)   # (without the clip box the staged march does run on this case)
    ren.set_lds_staging(True); ren.commit(); ren.render()
    assert ren.stats().lds_rounds > 0
    ren.close()


def test_invariant_device_group(ovr, oracle, hip_renderer_factory):
    case = _inv_case(ovr, oracle, size=(97, 61))

    def run(ren):
        _clipped(ovr, ren, case, accumulate=True)
        ren.commit()
        for _ in range(2):
            ren.render()
        a = hip_frame(ovr, ren) + (_counters(ren.stats()),)
        ren.set_clip_box((0.0, 8.0, -INF), (20.0, INF, 24.5))   # forwarded to every member, resets every member's accumulation
        ren.commit()
        ren.render()
        assert ren.stats().frame_index == 1
        return a, hip_frame(ovr, ren) + (_counters(ren.stats()),), ren.clip_box()

    single = hip_renderer_factory()
    want = run(single)
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        got = run(group)
    finally:
        group.close()
    for k in range(2):
        assert _bits_equal(got[k][0], want[k][0]) and _bits_equal(got[k][1], want[k][1]), k
        assert got[k][2] == want[k][2], k
    assert list(got[2].object_lower) == list(want[2].object_lower) and list(got[2].object_upper) == list(want[2].object_upper) and got[2].enabled == 1
    assert not np.array_equal(want[0][0], want[1][0])
    single.close()


@pytest.mark.parametrize("cam", ["oblique", "axis"])
def test_invariant_host_mirror_equals_the_device_frame(ovr, oracle, hip_renderer_factory, cam):
    """mapframe(HOST) copies the rectangle of the VOLUME's silhouette - a superset of the clip box's.  The axis camera at 48 x 17 pixels has a centre row whose
    rays have a y component of exactly 0: their y slab is ignored, and with the camera's y = 16 outside the box's [16.5, 20.25] they hit the clip box from
    outside its slab - the march counts those hits against the CLIP box's bounds, and such a frame is mapped whole"""
    case = _inv_case(ovr, oracle)
    if cam == "axis":
        case = dict(_inv_case(ovr, oracle, tf="dense"), cam=(CAMERAS["axis"][0], CAMERAS["axis"][1], (0.0, 1.0, 0.0)), fovy=40.0, size=(48, 17))
    box = BOX if cam == "oblique" else ((5.5, 16.5, 9.0), (27.0, 20.25, INF))
    ren = _clipped(ovr, hip_renderer_factory(), case, box=box)
    ren.commit()
    ren.render()
    fb_h, fb_d = ovr.FrameBufferData(), ovr.FrameBufferData()
    ren.mapframe(fb_h)
    ren.mapframe(fb_d, device=True)
    h = np.array(fb_h.rgba.data(), copy=True)
    d = fb_d.rgba.data().cpu().numpy().reshape(h.shape)
    assert _bits_equal(h, d) and h[..., 3].max() > 0
    if cam == "axis":   # the centre row, sy = 8.5 / 17 = 0.5 exactly: lit through the ignored slab although the row below it passes under the box
        assert (h[8, :, 3] > 0).sum() >= 3 and (h[7, :, 3] == 0).all()
    ren.close()


def test_invariant_combined_with_light_and_material(ovr, oracle, hip_renderer_factory):
    case = _inv_case(ovr, oracle)
    frames = {}
    for pipeline in (1, 2):
        for skip in (False, True):
            ren = _clipped(ovr, hip_renderer_factory(), case, pipeline=pipeline)
            ren.set_light_direction((1.0, -1.0, 0.3), 1.3)
            ren.set_material(0.6, 0.9, 0.4, 40.0)
            ren.set_empty_space_skipping(skip)
            ren.commit()
            ren.render()
            st = ren.stats()
            frames[(pipeline, skip)] = hip_frame(ovr, ren) + ((st.rays, st.samples + st.skipped_samples, st.shaded_samples, st.shadow_samples + st.skipped_shadow_samples),)
            ren.close()
    lit = _same(frames)
    ren = _clipped(ovr, hip_renderer_factory(), case, pipeline=1)
    ren.commit(); ren.render()
    ref = hip_frame(ovr, ren)
    ren.close()
    assert np.abs(lit[0] - ref[0]).max() > 0.05 and _bits_equal(lit[0][..., 3], ref[0][..., 3])   # another shade, the same alpha


# ---- 6. neutral element and empty box -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("pipeline", [1, 2])
def test_a_box_that_contains_the_volume_changes_nothing(ovr, oracle, hip_renderer_factory, pipeline, skip):
    case = _inv_case(ovr, oracle, n=40)
    variants = {"never called": None, "margin 1": ((-1.0, -1.0, -1.0), (41.0, 41.0, 41.0)), "all open": ((-INF,) * 3, (INF,) * 3)}
    got = {}
    for name, box in variants.items():
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        ren.set_empty_space_skipping(skip)
        if box is not None:
            ren.set_clip_box(*box)
        ren.commit()
        ren.render()
        st = ren.stats()
        got[name] = hip_frame(ovr, ren) + (_counters(st) + (st.pipeline, st.layout, st.skipping_kernels, st.lds_rounds),)
        assert ren.clip_box().enabled == (box is not None)
        assert list(ren.clip_box().object_lower) == [0.0] * 3 and list(ren.clip_box().object_upper) == [1.0] * 3
        ren.close()
    base = _same(got)
    assert base[0][..., :3].max() > 0.1 and base[2][1] > 0


@pytest.mark.parametrize("box", [((3.0, 0.0, 0.0), (3.0, 32.0, 32.0)), ((33.0, 33.0, 33.0), (40.0, 40.0, 40.0)), ((0.0, 40.0, 0.0), (32.0, 41.0, 32.0))], ids=["flat", "beside", "above"])
def test_an_empty_box_gives_a_zero_frame(ovr, oracle, hip_renderer_factory, box):
    case = _inv_case(ovr, oracle, cam="front")   # the front camera's centre column / row has exact zero direction components: ignored slabs
    for pipeline in (1, 2):
        for setup in ("dense", "accumulate", "sparse"):
            ren = _clipped(ovr, hip_renderer_factory(), case, box=box, pipeline=pipeline, accumulate=setup == "accumulate")
            if setup == "sparse":
                ren.set_noise_tile((np.random.default_rng(11).integers(0, 256, size=(32, 32, 64)) / 255.0).astype(F))
                ren.set_sparse_sampling(True)
            ren.commit()
            ren.render()
            rgba, grad = hip_frame(ovr, ren)
            st = ren.stats()
            assert not rgba.any() and not grad.any(), (pipeline, setup)
            assert st.samples == 0 and st.shaded_samples == 0 and st.shadow_samples == 0 and st.skipped_samples == 0
            assert st.rays == st.active_pixels > 0 and (setup == "sparse" or st.rays == 96 * 64)
            ren.close()


# ---- 7. the state machine -------------------------------------------------------------------------------------------------------------------------

def test_state_machine(ovr, oracle, hip_renderer_factory):
    clipping = ovr.clipping
    case = _inv_case(ovr, oracle, tf="dense", size=(64, 48))
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    ren.set_convergence(2, 0.0)          # adaptive; one sample per pixel without jitter: the error is 0 and every block retires with the first estimate
    ren.commit()
    c0 = ren.clip_box()
    assert c0.enabled == 0 and list(c0.lower) == [-INF] * 3 and list(c0.upper) == [INF] * 3 and list(c0.object_lower) == [0.0] * 3 and list(c0.object_upper) == [1.0] * 3
    for box in (BOX, ((0.0, 0.0, 0.0), (16.0, 32.0, 32.0)), None):
        while ren.stats().frame_index < 4:
            ren.render()
        conv = ren.convergence()
        assert ren.stats().frame_index == 4 and conv.valid == 1 and conv.retired_blocks > 0
        before = hip_frame(ovr, ren)[0]
        was = ren.clip_box()
        if box is None:
            ren.set_clip_box(None)
        else:
            ren.set_clip_box(*box)
        ren.render()                      # queued: nothing happens before the commit
        assert ren.stats().frame_index == 5
        now = ren.clip_box()              # ... and the getter reports the committed box, not the queued one
        assert (now.enabled, list(now.lower), list(now.upper), list(now.object_lower)) == (was.enabled, list(was.lower), list(was.upper), list(was.object_lower))
        ren.commit()
        conv = ren.convergence()
        assert conv.valid == 0 and conv.retired_blocks == 0
        now = ren.clip_box()
        assert now.enabled == (box is not None)
        if box is not None:
            assert list(now.lower) == [float(F(x)) for x in box[0]] and list(now.upper) == [float(F(x)) for x in box[1]]
        ren.render()
        assert ren.stats().frame_index == 1
        assert not np.array_equal(hip_frame(ovr, ren)[0], before)
    # the same value again: nothing changed, nothing is reset
    ren.set_clip_box(*BOX); ren.commit(); ren.render(); ren.render()
    assert ren.stats().frame_index == 2
    ren.set_clip_box(*BOX); ren.commit(); ren.render()
    assert ren.stats().frame_index == 3
    # EINVAL leaves the state and the accumulation alone
    frame = hip_frame(ovr, ren)[0]
    nan = float("nan")
    L = ovr._lib
    h, lib = ren._h, L.load()
    f3 = lambda v: (L.C.c_float * 3)(*v)
    for lo, hi in (((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, nan, 1)), ((2, 0, 0), (1, 1, 1)), ((0, 0, INF), (1, 1, 0))):
        with pytest.raises(RuntimeError, match="ovr_hip_set_clip_box"):
            ren.set_clip_box(lo, hi)
    assert lib.ovr_hip_set_clip_box(h, f3((0, 0, 0)), None) == -1 and b"ovr_hip_set_clip_box" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_set_clip_box(h, None, f3((1, 1, 1))) == -1
    ren.commit()                          # nothing was queued by the refused calls
    ren.render()
    assert ren.stats().frame_index == 4
    s = ren.clip_box()
    assert s.enabled == 1 and list(s.lower) == [float(F(x)) for x in BOX[0]] and list(s.upper) == [float(F(x)) for x in BOX[1]]
    # a new volume with other spacing recomputes the object box
    inv, wp = clipping.volume_constants((32, 32, 32))
    lo, hi = clipping.object_box(BOX[0], BOX[1], inv, wp)
    assert _bits_equal(np.array(list(s.object_lower), F), lo) and _bits_equal(np.array(list(s.object_upper), F), hi)
    assert [float(x) for x in lo] == [5.5 / 32, 0.0, 9.0 / 32] and [float(x) for x in hi] == [27.0 / 32, 20.25 / 32, 1.0]
    other = make_case(ovr, oracle, n=0, dims=(40, 23, 31), spacing=(1.0, 1.5, 0.75), origin=(3.0, -2.0, 5.0), tf="dense", cam="oblique", size=(64, 48), shading=2)
    ren.set_scene(ovr.Scene(volume=other["vol"], grid_origin=other["origin"], grid_spacing=other["spacing"], transfer_function=None))
    ren._upload_volume(ren.current_scene)
    ren.commit()
    s = ren.clip_box()
    inv, wp = clipping.volume_constants((40, 23, 31), (1.0, 1.5, 0.75), (3.0, -2.0, 5.0))
    lo, hi = clipping.object_box(BOX[0], BOX[1], inv, wp)
    assert _bits_equal(np.array(list(s.object_lower), F), lo) and _bits_equal(np.array(list(s.object_upper), F), hi)
    ren.set_grid_convention(1)            # ... and so does another grid convention
    ren.commit()
    s = ren.clip_box()
    inv, wp = clipping.volume_constants((40, 23, 31), (1.0, 1.5, 0.75), (3.0, -2.0, 5.0), vertex_centred=True)
    lo, hi = clipping.object_box(BOX[0], BOX[1], inv, wp)
    assert _bits_equal(np.array(list(s.object_lower), F), lo) and _bits_equal(np.array(list(s.object_upper), F), hi)
    ren.render()
    assert ren.stats().frame_index == 1 and ren.stats().samples > 0
    ren.close()


def test_never_calling_the_setter_leaves_the_stats_untouched(ovr, oracle, hip_renderer_factory):
    """ovr_hip_stats did not change: the same struct, and a renderer on which the setter was never called reports what one with the box removed again does"""
    case = _inv_case(ovr, oracle)
    a = hip_setup(ovr, hip_renderer_factory(), case, pipeline=2)
    a.render()
    b = _clipped(ovr, hip_renderer_factory(), case, pipeline=2)
    b.commit(); b.render()
    b.set_clip_box(None); b.commit(); b.render()
    sa, sb = a.stats(), b.stats()
    assert _counters(sa) == _counters(sb) and (sa.pipeline, sa.layout, sa.lds_rounds) == (sb.pipeline, sb.layout, sb.lds_rounds)
    assert _bits_equal(hip_frame(ovr, a)[0], hip_frame(ovr, b)[0])
    a.close(); b.close()


def test_a_box_change_voids_the_tuners_measurement(ovr, oracle, hip_renderer_factory):
    """as tests/test_lighting_gpu.py::test_a_light_change_voids_the_tuners_measurement for the light: a cut volume is another workload"""
    case = make_case(ovr, oracle, n=48, tf="dense", cam="front", size=(96, 64), shading=2, rate=2.0)
    ren = hip_renderer_factory()
    ren.set_volume_layouts(2)
    hip_setup(ovr, ren, case)
    seen = []
    for _ in range(14):
        ren.render()
        seen.append(ren.stats().tuning)
    assert seen[-1] == 2 and 1 in seen, seen
    ren.set_clip_box((0.0, 0.0, 0.0), (24.0, 48.0, 48.0))
    ren.commit()
    ren.render()
    assert ren.stats().tuning == 0
    for _ in range(4):                      # ... and it measures again
        ren.render()
        if ren.stats().tuning == 1:
            break
    assert ren.stats().tuning == 1
    ren.set_clip_box((0.0, 0.0, 0.0), (24.0, 48.0, 48.0))   # the same box during the probe: nothing is voided
    ren.commit()
    ren.render()
    assert ren.stats().tuning == 1
    ren.set_clip_box(None)                  # another one is
    ren.commit()
    ren.render()
    assert ren.stats().tuning == 0
    ren.close()


# ---- 8. the drop-in plugin ------------------------------------------------------------------------------------------------------------------------

def test_renderbatch_clip_box_variable(tmp_path, ovr, oracle, hip_renderer_factory):
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
    for k in ("OVR_HIP_CLIP_BOX", "OVR_HIP_QUIET"):
        env0.pop(k, None)

    def batch(tag, **extra):
        out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / tag)],
                             env=dict(env0, **extra), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        return np.asarray(Image.open(str(tmp_path / f"{tag}000000.png")).convert("RGBA")), out.stderr

    plain, err = batch("plain")
    assert "[hip] clip box" not in err
    cut, err = batch("cut", OVR_HIP_CLIP_BOX="8,-inf,10.5,40,24,inf")
    assert "[hip] clip box (8, -inf, 10.5) .. (40, 24, inf)" in err
    _, err_quiet = batch("quiet", OVR_HIP_CLIP_BOX="8,-inf,10.5,40,24,inf", OVR_HIP_QUIET="1")
    assert "[hip] clip box" not in err_quiet

    def host(box):
        scene, camera = ovr.vidi3d.scene_from_file(scene_path)
        assert scene.clipping_box is None
        ren = hip_renderer_factory()
        ren.set_fbsize((W, H))
        ren.set_frame_accumulation(True)
        ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
        ren.init(scene, camera)
        ren.set_camera(camera.eye, camera.at, camera.up)   # fovy 60 (renderer.h:149-152)
        if box:
            ren.set_clip_box(*box)
        ren.commit()
        ren.render()
        return oracle.rgba8(hip_frame(ovr, ren)[0], flip=True).reshape(H, W, 4)

    want_plain, want_cut = host(None), host(((8.0, -INF, 10.5), (40.0, 24.0, INF)))
    assert np.abs(plain.astype(int) - want_plain.astype(int)).max() <= 1
    assert np.abs(cut.astype(int) - want_cut.astype(int)).max() <= 1
    assert np.abs(cut.astype(int) - plain.astype(int)).max() > 20
