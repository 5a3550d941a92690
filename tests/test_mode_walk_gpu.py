"""The walk of tests/mode_walk.py on the GPU: march -> projection -> isosurfaces -> translucent isosurfaces -> march on ONE renderer, with camera kind, clip box,
shadow cache, light, material, ovr_hip_update_volume, skipping, layouts, pipeline, convergence, sparse sampling, reconstruction, frame size, transfer
function, new volumes, swaps and shards changing in between - and every checked frame (the first one behind a commit and the last one) held to

  A. its definition, where a whole-frame definition exists (mode_walk.has_definition): the CPU oracle for a plain march, by the bar of tests/fuzz_states.py;
     projection.frame / isosurface.frame for the other kinds, by the _check_frame of tests/test_projection_gpu.py, tests/test_isosurface_gpu.py and
     tests/test_isosurface_layers_gpu.py - the same functions, imported;
  B. its fresh twin, always: a second renderer created for the check, given the current volume (patches applied on the host) and the current state through
     one canonical setter sequence, one commit, and the frames and swaps the walked renderer has seen since its accumulation last started over.  RGBA and
     layer bit for bit, the counters that no kernel variant changes equal.

and to the predicted ovr_hip_stats.frame_index, the host mirror and - one check in four - the device's 8-bit conversion.  Hunts what the feature tests, each on
a fresh renderer, cannot see: state a frame kind leaves behind for the next one (schedule, block lists, clear generation, mapped rectangle, value ranges,
lattice, retired blocks, tuner and skipping probe)."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import mode_walk as W
from helpers import EXACT_RUN, compare, hip_frame
from test_isosurface_gpu import _check_frame as check_isosurface_frame
from test_isosurface_layers_gpu import _check_frame as check_layers_frame
from test_projection_gpu import _check_frame as check_projection_frame

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
GROUP_DEVICES = [0, 0, 0]
TWIN_COUNTERS = ("rays", "active_pixels", "samples + skipped_samples", "shaded_samples", "shadow_samples + skipped_shadow_samples")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _twin_counters(st):
    return (st.rays, st.active_pixels, st.samples + st.skipped_samples, st.shaded_samples, st.shadow_samples + st.skipped_shadow_samples)


def _camera(ovr, s):
    return ovr.Camera(s["eye"], s["at"], s["up"], s["fovy"], orthographic_height=s["ortho"])


def _scene(ovr, s):
    return ovr.Scene(volume=W.volume_of(s), grid_origin=(0.0, 0.0, 0.0), grid_spacing=(1.0, 1.0, 1.0), transfer_function=None, volume_sampling_rate=s["rate"])


def apply_state(ovr, ren, s):
    """the canonical setter sequence: the complete state, the volume upload, ONE commit (init's)"""
    colors, alphas, vr = W.tfn_of(ovr, s)
    ren.set_volume_layouts(2)
    ren.set_noise_tile(W.noise_tile())
    ren.set_fbsize(s["size"])
    ren.set_frame_accumulation(s["accumulate"])
    ren.set_sample_per_pixel(s["spp"])
    ren.set_volume_sampling_rate(s["rate"])
    ren.set_shading(s["shading"])
    ren.set_shading_pipeline(s["pipeline"])
    ren.set_grid_convention(0)
    ren.set_transfer_function(colors, alphas, vr)
    ren.set_pixel_jitter(s["jitter"])
    ren.set_focus(*s["focus"])
    ren.set_sparse_sampling(s["sparse"])
    ren.set_light_direction(*s["light"])
    ren.set_material(*s["material"])
    if s["clip"] is not None:
        ren.set_clip_box(*s["clip"])
    ren.set_shadow_cache(*s["shadow"])
    ren.set_projection(s["projection"])
    ren.set_isosurfaces(s["iso"], s["opacities"])
    ren.set_empty_space_skipping(s["skipping"])
    ren.set_layout_choice(s["layout"])
    ren.set_lds_staging(s["lds"])
    ren.set_convergence(*s["convergence"])
    ren.set_reconstruction(s["reconstruction"])
    if s["shard"]:
        ren.set_image_shard(*s["shard"])
    ren.init(_scene(ovr, s), _camera(ovr, s))


def apply_call(ovr, ren, call, s):
    """one setter call of a transition on the walked renderer; s: the state behind the transition"""
    name, args = call[0], call[1:]
    if name == "set_camera":
        ren.set_camera(_camera(ovr, s))
    elif name == "set_transfer_function":
        ren.set_transfer_function(*W.tfn_of(ovr, s))
    elif name == "set_focus":
        ren.set_focus(*args)
    elif name == "set_clip_box":
        ren.set_clip_box(None) if args[0] is None else ren.set_clip_box(*args)
    elif name == "update_volume":
        ren.update_volume(W.patch_array(s, args), args[0])
    elif name == "new_volume":   # the application's "open file", as tests/fuzz_states.py does it
        ren.set_transfer_function(*W.tfn_of(ovr, s))
        ren.init(_scene(ovr, s), _camera(ovr, s))
        ren.set_sparse_sampling(s["sparse"])
    else:
        getattr(ren, name)(*args)


def _masked(a, mask):
    return a if mask is None else np.where(mask[..., None], a, 0.0).astype(np.float32)


def _worst(got, ref):
    d = np.abs(got - ref)
    d = np.where(np.isnan(d), np.inf, d)
    y, x, ch = np.unravel_index(int(np.argmax(d)), d.shape)
    return f"worst pixel ({x},{y}) channel {ch}: walked {got[y, x]} reference {ref[y, x]}; {int((_bits(got) != _bits(ref)).any(-1).sum())} pixels differ"


def check_definition(ovr, O, s, c, got, layer, st, tag):
    """reference A"""
    mask = W.owned_mask(ovr, s)
    if W.frame_kind(s) == "march":   # tests/fuzz_states.py::check, the tolerance for low-alpha pixels as written out there
        ref, cnt = W.march_definition(ovr, O, s, c["frame_index"])
        got, ref = _masked(got, mask), _masked(ref, mask)
        try:
            compare(O, got, ref, name=tag)
        except AssertionError as e:
            # the known ill-conditioning of the reference's un-premultiplied output: a pixel with alpha of a few thousandths
            # may miss the float bar in `color / alpha` while alpha and the premultiplied colour - what the pixel shows - agree
            dd = np.abs(got - ref)
            pm = np.abs(got[..., :3] * got[..., 3:4] - ref[..., :3] * ref[..., 3:4])
            off = dd[..., :3].max(axis=-1) > 2e-4
            tolerated = not EXACT_RUN and not np.isnan(got).any() and dd[..., 3].max() <= 2e-4 and pm.max() <= 2e-4 and (ref[..., 3][off] < 0.02).all() and dd[..., :3].max() <= 2e-3
            if not tolerated:
                raise AssertionError(f"A: {e}; {_worst(got, ref)}; layout {st.layout} pipeline {st.pipeline}")
        assert st.samples + st.skipped_samples == cnt.samples, (tag, "A: samples", st.samples, st.skipped_samples, cnt.samples)
        return
    want = W.model_definition(ovr, s, W.model_frame_index(s, c["frame_index"]), exact=EXACT_RUN)
    case = W.case_of(ovr, s)
    try:
        if W.frame_kind(s) == "projection":
            check_projection_frame(case, (got, layer, st), want, tag)
        elif W.frame_kind(s) == "isosurface":
            check_isosurface_frame(O, case, (got, layer, st), want, tag, skipping=s["skipping"])
        else:
            check_layers_frame(O, case, (got, layer, st), want, tag, skipping=s["skipping"])
    except AssertionError as e:
        raise AssertionError(f"A: {e}; rgba {_worst(got, want[0])}; layer {_worst(layer, want[1])}")


def check_twin(ovr, make, s, c, got, layer, st, tag):
    """reference B"""
    twin = make()
    try:
        apply_state(ovr, twin, s)
        for h in c["history"]:   # the swaps and frames since the walked renderer's accumulation last started over
            twin.swap() if h == "s" else twin.render()
        t_rgba, t_layer = hip_frame(ovr, twin)
        ts = twin.stats()
    finally:
        twin.close()
    assert ts.frame_index == c["frame_index"], (tag, "B: the twin's own frame_index", ts.frame_index, c["frame_index"])
    mask = W.owned_mask(ovr, s)
    a, b = _masked(got, mask), _masked(t_rgba, mask)
    assert np.array_equal(_bits(a), _bits(b)), f"{tag} B: rgba differs from the fresh twin's; {_worst(a, b)}; walked layout {st.layout} pipeline {st.pipeline} tuning {st.tuning}, twin {ts.layout} {ts.pipeline} {ts.tuning}"
    a, b = _masked(layer, mask), _masked(t_layer, mask)
    assert np.array_equal(_bits(a), _bits(b)), f"{tag} B: layer differs from the fresh twin's; {_worst(a, b)}"
    assert _twin_counters(st) == _twin_counters(ts), (tag, "B: counters", TWIN_COUNTERS, _twin_counters(st), _twin_counters(ts))


def run_episode(ovr, O, make, ep, group):
    e = W.episode(W.SEED, ep, group, W.GROUP_EPISODES if group else W.EPISODES)
    log, checked = [], [0]
    ren = make()

    def check(t, c, tag):
        s = t["state"]
        got, layer = hip_frame(ovr, ren)
        st = ren.stats()
        log.append(f"    checked frame {c['after']}: frame_index {st.frame_index} layout {st.layout} pipeline {st.pipeline} tuning {st.tuning} reference {'A, B' if c['definition'] else 'B'}")
        assert st.frame_index == c["frame_index"], (tag, "frame_index", st.frame_index, "predicted", c["frame_index"])
        fbd = ovr.FrameBufferData()
        ren.mapframe(fbd, device=True)   # the host mirror is a copy of the device frame - of ALL of it, whatever rectangle was refreshed
        for lay, host in (("rgba", got), ("grad", layer)):
            dev = getattr(fbd, lay).data().cpu().numpy().reshape(host.shape)
            assert np.array_equal(_bits(dev), _bits(host)), f"{tag} host mirror != device frame ({lay}); {_worst(host, dev)}"
        if checked[0] % 4 == 0:          # the 8-bit frame the device converts (image_to_rgba8), flipped like the PNG writer wants it
            want = O.rgba8(got, flip=True)
            assert np.array_equal(np.array(ren.mapframe_rgba8(flip_vertical=True), copy=True).reshape(want.shape), want), tag + " rgba8"
        checked[0] += 1
        if c["definition"]:
            check_definition(ovr, O, s, c, got, layer, st, tag)
        check_twin(ovr, make, s, c, got, layer, st, tag)

    try:
        t = e["initial"]
        log.append(f"init {t['state']}")
        apply_state(ovr, ren, t["state"])
        ren.render()
        check(t, t["checks"][0], f"episode {ep} initial")
        for k, t in enumerate(e["transitions"]):
            log.append(W.describe(t))
            for call in t["calls"]:
                apply_call(ovr, ren, call, t["state"])
            ren.commit()
            marks = {c["after"]: c for c in t["checks"]}
            for n in range(1, t["frames"] + 1):
                ren.render()
                if n in marks:
                    check(t, marks[n], f"episode {ep} transition {k} ({'+'.join(t['labels'])}) frame {n}")
    except AssertionError as err:
        pytest.fail(f"episode {ep} (seed {W.SEED}{', group' if group else ''}): {str(err)[:1500]}\n" + "\n".join("   " + line for line in log), pytrace=False)
    finally:
        ren.close()
    return checked[0]


@pytest.mark.parametrize("ep", range(W.EPISODES), ids=lambda n: f"ep{n:02d}")
def test_walk_single(ovr, oracle, hip_renderer_factory, ep):
    t0 = time.time()
    n = run_episode(ovr, oracle, hip_renderer_factory, ep, False)
    print(f"episode {ep}: {n} checked frames in {time.time() - t0:.2f} s")


@pytest.mark.parametrize("ep", range(W.GROUP_EPISODES), ids=lambda n: f"ep{n:02d}")
def test_walk_device_group(ovr, oracle, ep):
    """the same walk on an in-process device group of three members on device 0: every frame is the whole frame; FILL is replaced by OFF (the header refuses it)"""
    made = []

    def make():
        made.append(ovr.create_renderer("hip", devices=GROUP_DEVICES))
        return made[-1]

    t0 = time.time()
    try:
        n = run_episode(ovr, oracle, make, ep, True)
    finally:
        for r in made:
            r.close()
    print(f"group episode {ep}: {n} checked frames in {time.time() - t0:.2f} s")


def test_walk_is_exact_under_the_exact_parity_build():
    """started the way test_isosurfaces_are_exact_under_the_exact_parity_build starts its child: the first episodes under the exact-parity build of the
    kernels, where reference A is equality everywhere"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    wanted = " or ".join(f"ep{n:02d}" for n in range(W.EXACT_EPISODES))
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", f"test_walk_single and ({wanted})"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)   # (a killed child raises TimeoutExpired: a failure, never a retry)
    tail = out.stdout[-4000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == W.EXACT_EPISODES and "failed" not in out.stdout.splitlines()[-1], tail
