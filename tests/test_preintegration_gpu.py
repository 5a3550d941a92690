"""Pre-integrated classification on the GPU (include/ovr_hip.h ovr_hip_set_preintegration): pinned from one side by frames of the SAME
renderer - over a constant volume the pre-integrated frame is the SHADE_NONE march frame, bit for bit and in the product build - and everywhere else by the numpy
model open-volume-renderer_amd/preintegration.py, which tests/test_preintegration_model.py pins to the unmodified oracle, to a closed form and to the feature's
claim.  The models are fed the library's own node table (ovr_hip_get_preintegration_tables; tests/test_preintegration_host.py holds its builder to the model's).
"Bits" are float32 bit patterns.  The first branch goes through the opacity correction's pow and the integral branch through exp2: the product evaluates them
with v_exp_f32 / v_log_f32, so against the model it meets helpers.compare's float bar, and a ray with a loop test within 1e-5 of the termination threshold may
take a segment more or less; the product also normalises 8-bit voxels behind the filter, so a segment of such a volume whose fabs(du) * (M - 1) lies within 1e-4
of 1 may take the other branch.  The exact-parity library (test_exact_under_the_exact_parity_build starts this file with it) gives the model's bits and counters
for every type."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import preintegration_cases as QC
import projection_cases as PC
import signed_cases as SG
from helpers import EXACT_RUN, compare, hip_frame, hip_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
F = np.float32
INF = float("inf")
OFF, SEGMENTS = 0, 1
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
TOL = 2e-4   # helpers.compare's float bar
# every voxel type under the modes 0 ... 3; the row loads (mode 4) where the layout has them
MATRIX = [(d, am) for d in QC.DTYPES for am in SG.ADDRESSING if am != "rows" or np.dtype(d).itemsize <= 2]
_IDS = [f"{np.dtype(d).name}-{am}" for d, am in MATRIX]
CLIP = ((5.5, -INF, 3.0), (27.0, 20.25, INF))
CENTRE = (20.0, 16.5, 9.0)
_models = {}


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _case(ovr, vol, tf=QC.TF, cam=QC.CAMERA, rate=QC.RATE, shading=0, spp=1, size=PC.SIZE, volume_kind=QC.VOLUME):
    colors, alphas, vr = QC.transfer_function(ovr, tf, vol.dtype, volume_kind)
    return dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=PC.CAMERAS[cam], size=size, shading=shading, rate=rate, spp=spp, convention=0,
                spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=PC.FOVY)


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


def _model(ovr, ren, case, key=None, **kw):
    """the model's frame over the library's own node table; `key` caches it across the addressing modes (the frame does not depend on them)"""
    if key is not None and key in _models:
        return _models[key]
    ct, at, tfr = _tables(ovr, case)
    out = ovr.preintegration.frame(case["vol"], _basis(ren), case["size"], case["rate"], ct, at, tfr, nodes=ren.preintegration_tables(), **kw)
    if key is not None:
        _models[key] = out
    return out


def _same_frame(a, b, tag, counters=COUNTERS):
    assert _same(a[0], b[0]) and _same(a[1], b[1]), (tag, float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))
    assert [getattr(a[2], k) for k in counters] == [getattr(b[2], k) for k in counters], (tag, [(k, getattr(a[2], k), getattr(b[2], k)) for k in counters])


def _preintegrated_stats(st, tag):
    assert st.skipped_samples == 0 and st.shadow_samples == 0 and st.skipped_shadow_samples == 0 and st.layout == 0 and st.pipeline == 1 and st.tuning == 0, tag
    assert st.skipping_kernels == 0, tag


def _check_frame(ovr, oracle, case, got, want, tag):
    """a pre-integrated frame against the model's: bits and counters under the exact-parity library; in the product build the float bar on rgba and `samples`
    within the model's hinge count (the segments of the rays with a borderline loop test)"""
    rgba, layer, st = got
    ref, cnt = want
    _preintegrated_stats(st, tag)
    assert not layer.any(), tag      # the gradient layer is zero
    assert st.rays == cnt["rays"] and st.active_pixels == cnt["active_pixels"], tag
    print(tag, "samples", st.samples, cnt["samples"], "shaded", st.shaded_samples, cnt["shaded"], "integral", cnt["integral"], "hinge", cnt["hinge"], "borderline pixels",
          int(cnt["borderline"].sum()), "branch-borderline pixels", int(cnt["branch_borderline"].sum()), "max |rgba - model|", float(np.abs(rgba - ref).max()))
    if EXACT_RUN:
        assert _same(rgba, ref), (tag, float(np.abs(rgba - ref).max()))
        assert st.samples == cnt["samples"] and st.shaded_samples == cnt["shaded"], (tag, st.samples, st.shaded_samples, cnt)
        return
    compare(oracle, rgba, ref, TOL, name=str(tag))
    assert abs(int(st.samples) - cnt["samples"]) <= cnt["hinge"], (tag, st.samples, cnt["samples"], cnt["hinge"])


# ---- 1. a constant volume: the same renderer's SHADE_NONE march, in the product build ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_a_constant_volume_gives_the_march_frame(ovr, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = QC.constant_volume(dtype)
    for cam in sorted(PC.CAMERAS):
        case = _case(ovr, vol, tf="dense", cam=cam, rate=1.0)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        for rate, clip in ((1.0, None), (2.7, None), (0.5, CLIP)):
            ren.set_volume_sampling_rate(rate)
            ren.set_clip_box(*clip) if clip else ren.set_clip_box(None)
            ren.set_preintegration(OFF)
            ren.commit()
            assert ren.get_preintegration().mode == OFF and ren.get_preintegration().active == 0
            march = _render(ovr, ren)
            ren.set_preintegration(SEGMENTS)
            ren.commit()
            assert ren.get_preintegration().mode == SEGMENTS and ren.get_preintegration().active == 1
            pre = _render(ovr, ren)
            tag = (np.dtype(dtype).name, am, cam, rate, clip is not None)
            _same_frame(pre, march, tag)
            _preintegrated_stats(pre[2], tag)
            g = ren.get_preintegration()
            assert (g.nodes, g.subdivision) == (61, 4), (tag, g.nodes, g.subdivision)
            assert march[2].samples > 500 and march[2].shaded_samples == march[2].samples and not march[1].any() and (march[0][..., 3] > 0.5).sum() > 100, (tag, march[2].samples)
        ren.close()


# ---- 2. ovr_hip_preintegrated_floats against the model ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", QC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("am", (0, 1, 2, 3))
def test_preintegrated_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    monkeypatch.setenv("OVR_HIP_ADDRESSING", str(am))
    P = ovr.preintegration
    eight_bit = np.dtype(dtype).itemsize == 1
    for dims in PC.DIMS:
        org, d, kind = PC.ray_set(dims)
        for volume_kind, tf in (("smooth", "ones"), ("random", "dense"), ("smooth", "shell")):
            vol = QC.volume(volume_kind, dtype, dims)
            case = _case(ovr, vol, tf=tf, volume_kind=volume_kind)
            ct, at, tfr = _tables(ovr, case)
            ren = hip_setup(ovr, hip_renderer_factory(), case)
            ren.set_preintegration(SEGMENTS)
            for rate in QC.RATES:
                ren.set_volume_sampling_rate(rate)
                ren.commit()
                nodes = ren.preintegration_tables()
                assert len(nodes) == P.node_count(len(ct), len(at), 4)
                key = ("rays", np.dtype(dtype).name, dims, volume_kind, tf, rate)
                if key not in _models:
                    _models[key] = P.preintegrated_rays(vol, org, d, rate, ct, at, tfr, nodes=nodes, border=QC.BORDER, du_border=QC.DU_BORDER)
                want = _models[key]
                steps, integral, tx, rgba = ren.preintegrated_rays(org, d)
                tag = (am, np.dtype(dtype).name, dims, volume_kind, tf, rate)
                if EXACT_RUN:
                    assert np.array_equal(steps, want["steps"]) and np.array_equal(integral, want["integral"]) and _same(tx, want["tx"]), tag
                    assert _same(rgba, want["rgba"]), (tag, float(np.abs(rgba - want["rgba"]).max()))
                else:
                    # a ray's segment count hangs on the last bit of exp2 / pow wherever a loop test was borderline; for 8-bit voxels its branch counts (and,
                    # by the two classifications' difference, its colour) hang on the tap's last bits wherever a segment's spread was
                    counted = ~want["borderline"]
                    branch = counted & ~want["branch_borderline"] if eight_bit else counted
                    assert counted.sum() > 30 and branch.sum() > 30, tag      # (the dense table over the random volume at rate 2.7 leaves 33 of 92)
                    assert np.array_equal(steps[counted], want["steps"][counted]) and _same(tx[counted], want["tx"][counted]), tag
                    assert np.array_equal(integral[branch], want["integral"][branch]), tag
                    assert not np.isnan(rgba).any() and np.abs(rgba - want["rgba"])[branch].max() <= TOL, (tag, float(np.abs(rgba - want["rgba"])[branch].max()))
                assert not rgba[kind == "miss"].any() and (steps[kind == "miss"] == 0).all() and not tx[kind == "miss"].any(), tag
                assert (steps > 0).sum() > 50 and (integral > 0).sum() > 20, tag
            ren.close()


# ---- 3. frames against the model -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,am", MATRIX, ids=_IDS)
def test_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, dtype, am):
    SG.set_addressing(monkeypatch, am)
    vol = QC.volume(QC.VOLUME, dtype)
    name = np.dtype(dtype).name
    for cam in sorted(PC.CAMERAS):
        case = _case(ovr, vol, cam=cam)
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        ren.set_preintegration(SEGMENTS)
        ren.commit()
        got = _render(ovr, ren)
        want = _model(ovr, ren, case, key=("frame", name, cam))
        _check_frame(ovr, oracle, case, got, want, (name, am, cam))
        assert want[1]["integral"] > 300 and want[1]["samples"] - want[1]["integral"] > 300 and got[2].shaded_samples > 500
        assert (got[0][..., 3] >= 0.9999).sum() >= 20 and ((got[0][..., 3] > 0) & (got[0][..., 3] < 0.9999)).sum() >= 20      # saturated and partial rays
        ren.close()


# ---- 4. variants: the orthographic camera, a clip box, samples per pixel with jitter and accumulation ------------------------------------------------

def test_orthographic_frame_vs_model(ovr, oracle, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_camera(ovr.Camera((-31.5, 44.25, -39.0), CENTRE, (0.0, 1.0, 0.0), orthographic_height=40.0))
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    got = _render(ovr, ren)
    _check_frame(ovr, oracle, case, got, _model(ovr, ren, case, camera_kind=ovr.camera.ORTHOGRAPHIC), "orthographic")
    assert got[2].shaded_samples > 500
    ren.close()


def test_clipped_frame_vs_model(ovr, oracle, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.uint16)
    nz, ny, nx = vol.shape
    box = ovr.clipping.object_box(*CLIP, *ovr.clipping.volume_constants((nx, ny, nz)))
    case = _case(ovr, vol, cam="oblique", rate=2.7)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    whole = _render(ovr, ren)
    ren.set_clip_box(*CLIP)
    ren.commit()
    got = _render(ovr, ren)
    _check_frame(ovr, oracle, case, got, _model(ovr, ren, case, clip=box), "clip box, rate 2.7")
    assert not _same(got[0], whole[0]) and 500 < got[2].samples < whole[2].samples
    ren.close()


def test_accumulation_spp_and_jitter(ovr, oracle, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.float32)
    case = _case(ovr, vol, spp=2)
    noise = np.random.default_rng(77).random((16, 16, 64)).astype(F)
    ren = hip_renderer_factory()
    ren.set_noise_tile(noise)
    ren.set_pixel_jitter(1)
    hip_setup(ovr, ren, case, accumulate=True)
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    one = _render(ovr, ren)
    want1 = _model(ovr, ren, case, spp=2, noise=noise, frame_index=1)
    _check_frame(ovr, oracle, case, one, want1, "spp 2, frame 1")
    two = _render(ovr, ren)
    want2 = _model(ovr, ren, case, spp=2, noise=noise, frame_index=2)
    assert two[2].frame_index == 2 and not _same(want2[0], want1[0])
    # the accumulated frame: (A1 + A2) / 2 per channel, as write_pixel forms it
    acc = ((want1[0] + want2[0]).astype(F) / F(2)).astype(F)
    if EXACT_RUN:
        assert _same(two[0], acc) and two[2].samples == want2[1]["samples"]
    else:
        compare(oracle, two[0], acc, TOL, name="accumulated")
        assert abs(int(two[2].samples) - want2[1]["samples"]) <= want2[1]["hinge"] and two[2].rays == want2[1]["rays"]
    ren.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_off_segments_off_and_the_accumulation(ovr, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    first = _render(ovr, ren)
    g = ren.get_preintegration()
    assert (g.mode, g.active, g.nodes, g.subdivision) == (OFF, 0, 0, 0) and first[2].frame_index == 1
    assert _render(ovr, ren)[2].frame_index == 2
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    seg = _render(ovr, ren)
    g = ren.get_preintegration()
    assert (g.mode, g.active, g.nodes, g.subdivision) == (SEGMENTS, 1, 61, 4) and seg[2].frame_index == 1 and not _same(seg[0], first[0]) and seg[2].shaded_samples > 0
    assert _render(ovr, ren)[2].frame_index == 2
    ren.set_preintegration(SEGMENTS)      # the same value again: still a call - the accumulation starts over
    ren.commit()
    again = _render(ovr, ren)
    _same_frame(again, seg, "the same mode again")
    assert again[2].frame_index == 1
    ren.set_preintegration(OFF)
    ren.commit()
    back = _render(ovr, ren)
    _same_frame(back, first, "OFF -> SEGMENTS -> OFF", COUNTERS + ("pipeline",))      # (not `layout`: a replica built in the background since the first frame may draw the later march)
    assert ren.get_preintegration().active == 0 and back[2].frame_index == 1
    for mode in (2, -1):      # refused values leave the state alone (ValueError where the ABI says EINVAL)
        with pytest.raises(ValueError, match="ovr_hip_set_preintegration"):
            ren.set_preintegration(mode)
    ren.commit()
    assert ren.get_preintegration().mode == OFF and _render(ovr, ren)[2].frame_index == 2      # no call was recorded: the accumulation goes on
    ren.close()


def test_shading_keeps_the_mode_and_draws_the_shaded_march(ovr, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.float32)
    case = _case(ovr, vol, shading=1)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    g = ren.get_preintegration()
    assert (g.mode, g.active) == (SEGMENTS, 0)
    kept = _render(ovr, ren)
    twin = hip_setup(ovr, hip_renderer_factory(), case)      # a fresh renderer that never heard of pre-integration
    _same_frame(kept, _render(ovr, twin), "GRADIENT shading: the shaded march", COUNTERS + ("pipeline",))
    assert kept[1].any()      # (the shaded march writes its gradient layer)
    ren.set_shading(0)
    ren.commit()
    assert ren.get_preintegration().active == 1
    seg = _render(ovr, ren)
    assert not seg[1].any() and not _same(seg[0], kept[0])
    twin.close()
    ren.close()


def test_a_transfer_function_commit_rebuilds_the_table(ovr, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.float32)
    case = _case(ovr, vol, tf="dense")
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    dense = _render(ovr, ren)
    assert ren.get_preintegration().nodes == 61
    other = _case(ovr, vol, tf="shell")
    ren.set_transfer_function(other["colors"], other["alphas"], other["vr"])
    ren.commit()
    assert ren.get_preintegration().nodes == 0      # stale until the next pre-integrated frame (or the tables getter) rebuilds it
    shell = _render(ovr, ren)
    assert ren.get_preintegration().nodes == 253 and not _same(shell[0], dense[0])
    twin = hip_setup(ovr, hip_renderer_factory(), other)
    twin.set_preintegration(SEGMENTS)
    twin.commit()
    assert len(twin.preintegration_tables()) == 253 and twin.get_preintegration().nodes == 253      # built by the getter
    _same_frame(shell, _render(ovr, twin), "a twin with the final tables")
    assert _same(ren.preintegration_tables(), twin.preintegration_tables())
    model = ovr.preintegration.node_table(*PC.tables(other["colors"], other["alphas"]), 4)      # (one float32 ulp: tests/test_preintegration_host.py)
    assert np.abs(twin.preintegration_tables().view(np.int32).astype(np.int64) - model.view(np.int32)).max() <= 1
    twin.close()
    ren.close()


def test_the_other_frame_kinds_are_drawn_and_preintegration_resumes(ovr, hip_renderer_factory):
    vol = QC.volume(QC.VOLUME, np.float32)
    case = _case(ovr, vol)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    twin = hip_setup(ovr, hip_renderer_factory(), case)      # never hears of pre-integration
    ren.set_preintegration(SEGMENTS)
    ren.commit()
    seg = _render(ovr, ren)
    kinds = (("slices", lambda r, on: r.set_slices([(CENTRE, (0.0, 0.0, 1.0))] if on else None)),
             ("isovalues", lambda r, on: r.set_isosurfaces([0.5] if on else [])),
             ("projection", lambda r, on: r.set_projection(ovr.PROJECT_MAXIMUM if on else ovr.PROJECT_OFF)))
    for name, setter in kinds:
        for r in (ren, twin):
            setter(r, True)
            r.commit()
        g = ren.get_preintegration()
        assert (g.mode, g.active) == (SEGMENTS, 0), name
        a, b = _render(ovr, ren), _render(ovr, twin)
        _same_frame(a, b, name)
        assert a[0].any() and not _same(a[0], seg[0]), name
        for r in (ren, twin):
            setter(r, False)
            r.commit()
        assert ren.get_preintegration().active == 1, name
        _same_frame(_render(ovr, ren), seg, name + " off: pre-integration resumes")
    # errors of the known-answer entry
    import torch
    lib = ovr._lib.load()
    buf = torch.zeros(24, dtype=torch.float32, device=torch.device("cuda", 0))
    assert lib.ovr_hip_preintegrated_floats(twin._h, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1) < 0 and b"no pre-integration is committed (ovr_hip_set_preintegration)" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_preintegrated_floats(ren._h, None, buf.data_ptr(), buf.data_ptr(), 1) < 0 and b"bad arguments" in lib.ovr_hip_last_error()
    twin.close()
    ren.close()


# ---- 6. a device group ---------------------------------------------------------------------------------------------------------------------------------------------

def test_a_device_group_gives_the_single_renderers_frame(ovr, hip_renderer_factory):
    case = _case(ovr, QC.volume(QC.VOLUME, np.float32), size=(56, 40))

    def start(ren):
        hip_setup(ovr, ren, case)
        ren.set_preintegration(SEGMENTS)
        ren.commit()
        return ren

    single = start(hip_renderer_factory())
    whole = _render(ovr, single)
    group = ovr.create_renderer("hip", devices=[0, 0])
    try:
        g = _render(ovr, start(group))
        c = group.get_preintegration()
        assert _same(g[0], whole[0]) and _same(g[1], whole[1]) and (c.mode, c.active) == (SEGMENTS, 1)
        assert (g[2].rays, g[2].samples, g[2].shaded_samples, g[2].active_pixels) == (whole[2].rays, whole[2].samples, whole[2].shaded_samples, whole[2].active_pixels)
        with pytest.raises(ValueError):
            group.set_preintegration(3)
    finally:
        group.close()
    assert whole[2].shaded_samples > 500
    single.close()


# ---- 7. the exact-parity build -------------------------------------------------------------------------------------------------------------------------------------

def test_exact_under_the_exact_parity_build():
    """started the way tests/test_slice_context_gpu.py starts its child: with the exact-parity build of the kernels the known-answer entry and the frames give the
    model's bits and counters for every voxel type"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
           "preintegrated_floats_vs_model or test_frames_vs_model or orthographic_frame_vs_model or clipped_frame_vs_model or accumulation_spp_and_jitter"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == 4 * len(QC.DTYPES) + len(MATRIX) + 3 and "failed" not in out.stdout.splitlines()[-1], tail
