"""The signed voxel types (int8, int16) on the GPU in every walk-frame kernel and in the march's controls, under every addressing mode: OVR_HIP_ADDRESSING 0 ... 3
and the aligned 8-byte row loads (mode 4, OVR_HIP_ROW_LOADS=1).  Inputs: tests/signed_cases.py; tests/test_signed_types_model.py pins the models' signed branches
to the unmodified oracle and states why these comparisons discriminate (a tap without the int8 clamp of -128 to -127, or one that reads the voxels as
unsigned, changes what is compared here).

Every comparison is its family's: the _case, _start, _render, _model, _check_frame and _sampler of tests/test_projection_gpu.py, tests/test_isosurface_gpu.py,
tests/test_isosurface_layers_gpu.py and tests/test_ambient_occlusion_gpu.py, imported; the march's controls through the helpers of tests/test_clipping_gpu.py,
tests/test_camera_gpu.py, tests/test_lighting_gpu.py and tests/test_shadow_cache_gpu.py.  int16 is compared where uint16 is (bits), int8 follows each family's
uint8 rule (isosurface families: bits through isosurface.product_sampler; projections: the float bar, tm* left out), and the exact-parity child
(test_signed_int8_is_exact_under_the_exact_parity_build) demands bits for int8 wherever a model or the oracle is the reference.

The bodies take the voxel type as a parameter: tests/test_addressing_matrix_gpu.py runs them for uint16 and uint8 under the row loads."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import camera_cases as CC
import isosurface_cases as IC
import projection_cases as PC
import signed_cases as SC
import test_ambient_occlusion_gpu as TA
import test_camera_gpu as TK
import test_clipping_gpu as TC
import test_isosurface_gpu as TI
import test_isosurface_layers_gpu as TL
import test_lighting_gpu as TG
import test_projection_gpu as TP
import test_shadow_cache_gpu as TS
from helpers import EXACT_RUN, compare, hip_frame, hip_setup, oracle_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
F = np.float32
MAXIMUM, MINIMUM, MEAN = 1, 2, 3
COUNTERS = TP.COUNTERS
FRAME_ADDRESSING = ("default", "rows")
IDS = lambda d: np.dtype(d).name
_memo = {}


def _once(key, fn):
    """a reference computed once per key and shared between the addressing modes (read-only by convention)"""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _am(name):
    return None if name == "default" else name


def _dims_of(am):
    """both volumes for modes 0, 3 and the row loads, the first alone for 1 and 2 (which share the row loads' pair extraction and mode 3's 64-bit offsets)"""
    return SC.DIMS if am in (0, 3, "rows") else SC.DIMS[:1]


def _eight_bit(dtype):
    return np.dtype(dtype).itemsize == 1


def _frame_volume(kind, dtype):
    return SC.volume(kind, dtype) if SC.is_signed(dtype) else IC.volume(kind, dtype)


def _counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


def _name(dtype):
    return np.dtype(dtype).name


def check_projection_frame(case, got, want, name):
    """test_projection_gpu._check_frame; an int8 volume takes its uint8 rule (that function reads nothing of the volume but its type)"""
    if np.dtype(case["vol"].dtype) == np.int8:
        case = dict(case, vol=case["vol"].view(np.uint8))
    TP._check_frame(case, got, want, name)


# ---- 1. the known-answer entries -------------------------------------------------------------------------------------------------------------------

def project_floats_body(ovr, make, dtype, am):
    """the body of test_projection_gpu.test_project_floats_vs_model"""
    P = ovr.projection
    exact = not _eight_bit(dtype) or EXACT_RUN
    for dims in _dims_of(am):
        vol = SC.any_volume("random", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        ren = hip_setup(ovr, make(), TP._case(ovr, vol))
        assert ren.get_projection().mode == 0
        for rate in SC.RATES:
            ren.set_volume_sampling_rate(rate)
            ren.commit()
            for mode in (MAXIMUM, MINIMUM, MEAN):
                want = _once(("project", _name(dtype), dims, rate, mode), lambda: P.project_rays(vol, org, d, rate, mode))
                for skip in (False, True):
                    v, tm, steps, fetched = ren.project_rays(org, d, mode, skip)
                    name = (am, dims, rate, mode, skip)
                    assert np.array_equal(steps, want["steps"]), name
                    if exact:
                        assert TP._same(v, want["v"]) and TP._same(tm, want["tm"]), name
                    else:   # (tm* is not compared: see test_projection_gpu._check_frame)
                        assert np.abs(v - want["v"]).max() <= TP.TOL_U8, name
                    assert (fetched <= steps).all(), name
                    if not skip or mode == MEAN:
                        assert np.array_equal(fetched, steps), name
                    assert (steps[kind == "miss"] == 0).all() and (v[kind == "miss"] == 0).all()
        ren.close()


def isosurface_floats_body(ovr, make, dtype, am):
    """the body of test_isosurface_gpu.test_isosurface_floats_vs_model, on `ball` with the type's edge isovalues"""
    I = ovr.isosurface
    hits = 0
    iso = SC.edge_isovalues(dtype)
    for dims in _dims_of(am):
        vol = SC.any_volume("ball", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        ren = hip_setup(ovr, make(), TI._case(ovr, vol))
        ren.set_light_direction(TI.LIGHT, 1.0)
        ren.set_isosurfaces(iso[::-1])
        ren.commit()
        assert list(ren.get_isosurfaces().isovalues[:3]) == list(iso) and ren.get_isosurfaces().n == 3
        for rate in SC.RATES:
            ren.set_volume_sampling_rate(rate)
            ren.commit()
            want = _once(("isosurface", _name(dtype), dims, rate), lambda: I.trace_rays(vol, org, d, rate, iso, light=TI.LIGHT, sampler=TI._sampler(ovr, vol)))
            for skip in (False, True):
                got = ren.isosurface_rays(org, d, skip)
                name = (am, dims, rate, skip)
                assert np.array_equal(got["hit"], want["hit"]) and np.array_equal(got["steps"], want["steps"]), name
                assert TI._same(got["iso"], want["iso"]) and TI._same(got["t"], want["t"]) and TI._same(got["shadow"], want["shadow"]), name
                if EXACT_RUN:
                    assert TI._same(got["normal"], want["normal"]), name
                else:
                    assert np.allclose(got["normal"], want["normal"], rtol=0, atol=TI.TOL, equal_nan=True), (name, float(np.nanmax(np.abs(got["normal"] - want["normal"]))))
                assert not got["hit"][kind == "miss"].any() and (got["steps"][kind == "miss"] == 0).all()
            hits += int(want["hit"].sum())
        ren.close()
    assert hits > 40


def layer_floats_body(ovr, make, dtype, am):
    """the body of test_isosurface_layers_gpu.test_layer_floats_vs_model"""
    I = ovr.isosurface
    events = 0
    iso = SC.layer_isovalues(dtype)
    for dims in _dims_of(am):
        vol = SC.any_volume("ball", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        ren = hip_setup(ovr, make(), TL._case(ovr, vol))
        ren.set_light_direction(TL.LIGHT, 1.0)
        ren.set_isosurfaces(iso[::-1], TL.MIXED[::-1])
        ren.commit()
        s = ren.get_isosurface_layers()
        assert list(s.isovalues) == list(iso) and s.n == 4 and s.translucent == 1
        for rate in SC.RATES:
            ren.set_volume_sampling_rate(rate)
            ren.commit()
            want = _once(("layers", _name(dtype), dims, rate), lambda: I.trace_rays(vol, org, d, rate, iso, light=TL.LIGHT, sampler=TL._sampler(ovr, vol), opacities=TL.MIXED))
            for skip in (False, True):
                got = ren.isosurface_layer_rays(org, d, TL.MAX_EVENTS, skip)
                TL._check_rays(got, want, (am, dims, rate, skip))
                assert not got["events"][kind == "miss"].any() and (got["steps"][kind == "miss"] == 0).all()
            events += int(want["n_events"].sum())
        ren.close()
    assert events > 100, events


def ao_floats_body(ovr, make, dtype, am):
    """the body of test_ambient_occlusion_gpu.test_ao_floats_vs_model with K = 5 and two of the sixteen rotations: (rate 1, R = 3) and (rate 2.5, R = inf)"""
    I = ovr.isosurface
    K = 5
    iso = SC.layer_isovalues(dtype)
    occluded = events = 0
    for dims in _dims_of(am):
        vol = SC.any_volume("ball", dtype, dims)
        org, d, kind = PC.ray_set(dims)
        rot = np.where(np.arange(len(org)) & 1, 12, 3)
        ren = TA._start(ovr, make(), TA._case(ovr, vol), iso[::-1], TA.MIXED[::-1], ao=(K, 3.0))
        for rate, R in ((1.0, 3.0), (2.5, TA.INF)):
            ren.set_volume_sampling_rate(rate)
            ren.set_ambient_occlusion(K, R)
            ren.commit()
            table = ren.ambient_occlusion_directions()
            for skip in (False, True):
                want = _once(("ao", _name(dtype), dims, rate, R, skip),
                             lambda: I.trace_rays(vol, org, d, rate, iso, light=TA.LIGHT, sampler=TA._sampler(ovr, vol), opacities=TA.MIXED, skipping=skip, ao=(table, R, rot)))
                f = want["flat"]
                first = np.concatenate([[0], np.cumsum(want["n_events"])[:-1]])
                slot = np.arange(len(f["ray"])) - first[f["ray"]]
                for m in (3, 12):
                    rays = np.flatnonzero(rot == m)
                    got = ren.isosurface_ao_rays(org[rays], d[rays], m, TA.MAX_EVENTS, skip)
                    name = (am, dims, rate, R, skip, m)
                    assert np.array_equal(got["events"], want["n_events"][rays]) and TA._same(got["A"], want["A"][rays]), name
                    assert np.array_equal(got["steps"], want["steps"][rays]) and np.array_equal(got["shadow_steps"], want["shadow_steps"][rays]), name
                    keep = np.isin(f["ray"], rays) & (slot < TA.MAX_EVENTS)
                    r, e = np.searchsorted(rays, f["ray"][keep]), slot[keep]
                    assert np.array_equal(got["k"][r, e], f["k"][keep]), name
                    for key, mine in (("t", "t"), ("shadow", "shadow"), ("A_after", "A"), ("O", "O")):
                        assert TA._same(got[key][r, e], f[mine][keep]), (name, key)
                    if EXACT_RUN:
                        assert TA._same(got["normal"][r, e], f["normal"][keep]), name
                    else:
                        assert np.allclose(got["normal"][r, e], f["normal"][keep], rtol=0, atol=TA.TOL, equal_nan=True), name
                    full = want["n_events"][rays] <= TA.MAX_EVENTS
                    assert np.array_equal(got["ao_steps"][full], want["ao_steps"][rays][full]) and np.array_equal(got["ao_fetched"][full], want["ao_fetched"][rays][full]), name
                    empty = np.ones(got["O"].shape, bool)
                    empty[r, e] = False
                    assert not got["O"][empty].any() and not got["t"][empty].any(), (name, "the rest is zeros")
                if not skip:
                    occluded += int(((f["O"] > 0) & (f["O"] < 1)).sum())
                    events += len(f["O"])
        ren.close()
    assert events > 100 and occluded > 30, (events, occluded)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", SC.ADDRESSING, ids=str)
def test_project_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, am)
    project_floats_body(ovr, hip_renderer_factory, dtype, am)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", SC.ADDRESSING, ids=str)
def test_isosurface_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, am)
    isosurface_floats_body(ovr, hip_renderer_factory, dtype, am)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", SC.ADDRESSING, ids=str)
def test_layer_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, am)
    layer_floats_body(ovr, hip_renderer_factory, dtype, am)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", SC.ADDRESSING, ids=str)
def test_ao_floats_vs_model(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, am)
    ao_floats_body(ovr, hip_renderer_factory, dtype, am)


# ---- 2. frames against the models ------------------------------------------------------------------------------------------------------------------
# every body returns the frames it drew as (rgba, layer, counters): the addressing matrix compares them between the row loads on and off

def projection_frames_body(ovr, oracle, make, dtype, modes=(MAXIMUM, MINIMUM, MEAN), check=True):
    vol = _frame_volume("random", dtype)
    case = TP._case(ovr, vol, cam=SC.CAMERA, rate=SC.FRAME_RATE)
    ren = hip_setup(ovr, make(), case)
    out = []
    for mode in modes:
        ren.set_projection(mode)
        ren.commit()
        got = TP._render(ovr, ren)
        if check:
            check_projection_frame(case, got, TP._model(ovr, oracle, case, mode, "random"), (_name(dtype), mode))
            assert (got[1][..., 2] == 1).sum() > 100
        out.append((got[0], got[1], _counters(got[2])))
    ren.close()
    return out


def hit_mask_identity_body(ovr, make, dtype):
    """the body of test_isosurface_gpu.test_hit_mask_from_the_projections on `ball`, at every isovalue of the type below zero (and the type's other edges)"""
    vol = _frame_volume("ball", dtype)
    case = TI._case(ovr, vol, cam=SC.CAMERA, rate=SC.FRAME_RATE, shading=0)
    ren = hip_setup(ovr, make(), case)
    layers = {}
    for mode in (MAXIMUM, MINIMUM):
        ren.set_projection(mode)
        ren.commit()
        layers[mode] = TI._render(ovr, ren)[1]
    marched = layers[MAXIMUM][..., 2] == 1
    levels = list(SC.any_scaled(IC.ISOVALUES["ball"], dtype)) + list(SC.EDGES.get(np.dtype(dtype), {}).values())
    negative = hits = 0
    for iso in levels:
        ren.set_isosurfaces([iso])
        ren.commit()
        got = TI._render(ovr, ren)
        want = marched & (layers[MAXIMUM][..., 0] >= iso) & (layers[MINIMUM][..., 0] < iso)
        assert np.array_equal(got[1][..., 2] == 1, want), (_name(dtype), float(iso))
        assert (got[1][..., 0][want] == iso).all() and (got[0][..., 3] == want).all()
        negative += int(iso < 0)
        hits += int(want.sum()) if iso < 0 else 0
    assert not SC.is_signed(dtype) or (negative >= 3 and hits > 100), (negative, hits)
    ren.close()


def isosurface_frames_body(ovr, oracle, make, dtype, sets=("opaque", "edge"), shadings=(2, 1, 0), check=True):
    out = []
    for which in sets:
        iso = SC.edge_isovalues(dtype) if which == "edge" else SC.any_scaled(IC.NESTED["ball"][:2], dtype)
        vol = _frame_volume("ball", dtype)
        ren = None
        for shading in shadings:
            case = TI._case(ovr, vol, cam=SC.CAMERA, rate=SC.FRAME_RATE, shading=shading)
            if ren is None:
                ren = TI._start(ovr, make(), case, iso)
            else:
                ren.set_shading(shading)
                ren.commit()
            got = TI._render(ovr, ren)
            if check:
                TI._check_frame(oracle, case, got, TI._model(ovr, oracle, case, iso, "ball"), (_name(dtype), which, shading))
                assert (got[1][..., 2] == 1).sum() > 40 and (got[2].shadow_samples > 0) == (shading == 2)
            out.append((got[0], got[1], _counters(got[2])))
        ren.close()
    return out


def translucent_frame_body(ovr, oracle, make, dtype, check=True):
    vol = _frame_volume("ball", dtype)
    iso = SC.layer_isovalues(dtype)
    case = TL._case(ovr, vol, cam=SC.CAMERA, rate=SC.FRAME_RATE, shading=2)
    ren = TL._start(ovr, make(), case, iso, SC.MIXED)
    got = TL._render(ovr, ren)
    if check:
        TL._check_frame(oracle, case, got, TL._model(ovr, oracle, case, iso, SC.MIXED, "ball"), (_name(dtype), "translucent"))
        a = got[0][..., 3]
        assert ((a > 0) & (a < 1)).sum() > 10 and got[2].shaded_samples > 40
    ren.close()
    return [(got[0], got[1], _counters(got[2]))]


def ao_frame_body(ovr, oracle, make, dtype, check=True):
    vol = _frame_volume("ball", dtype)
    iso = SC.layer_isovalues(dtype)
    case = TA._case(ovr, vol, cam=SC.CAMERA, rate=SC.FRAME_RATE, shading=1, size=SC.SIZE)
    ren = TA._start(ovr, make(), case, iso, SC.MIXED, ao=SC.AO)
    got = TA._render(ovr, ren)
    if check:
        want = _once(("ao frame", _name(dtype)), lambda: TA._model(ovr, oracle, case, iso, SC.MIXED, ren))      # (frame 1 under the host's table, whatever the addressing)
        assert got[2].frame_index == 1
        TA._check_frame(oracle, case, got, want, (_name(dtype), "ao"))
        assert want[2]["ao_steps"] > want[2]["hits"] > 40 and ren.get_ambient_occlusion().active == 1
    ren.close()
    return [(got[0], got[1], _counters(got[2]))]


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", FRAME_ADDRESSING)
def test_projection_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, _am(am))
    projection_frames_body(ovr, oracle, hip_renderer_factory, dtype)
    hit_mask_identity_body(ovr, hip_renderer_factory, dtype)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", FRAME_ADDRESSING)
def test_isosurface_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, _am(am))
    isosurface_frames_body(ovr, oracle, hip_renderer_factory, dtype)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", FRAME_ADDRESSING)
def test_translucent_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, _am(am))
    translucent_frame_body(ovr, oracle, hip_renderer_factory, dtype)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", FRAME_ADDRESSING)
def test_ao_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, am, dtype):
    SC.set_addressing(monkeypatch, _am(am))
    ao_frame_body(ovr, oracle, hip_renderer_factory, dtype)


@pytest.mark.parametrize("am", FRAME_ADDRESSING)
def test_all_minimum_isovalue_frames_vs_model(ovr, oracle, hip_renderer_factory, monkeypatch, am):
    """int8, the isovalue -1.0: every sample is on or above it - no hit pixel, the whole of every ray walked; the counters are the model's"""
    SC.set_addressing(monkeypatch, _am(am))
    vol = SC.volume("ball", np.int8)
    iso = [SC.INT8_EDGES["all_minimum"]]
    for skip in (False, True):
        case = TI._case(ovr, vol, cam=SC.CAMERA, rate=SC.FRAME_RATE, shading=2)
        ren = TI._start(ovr, hip_renderer_factory(), case, iso, skipping=skip)
        got = TI._render(ovr, ren)
        want = TI._model(ovr, oracle, case, iso, "ball", skipping=skip)
        TI._check_frame(oracle, case, got, want, ("all minimum", skip), skipping=skip)
        assert not got[0].any() and not got[1].any() and got[2].shaded_samples == 0 and want[2]["hits"] == 0 and want[2]["steps"] > 1000
        ren.close()


def test_signed_int8_is_exact_under_the_exact_parity_build():
    """started the way test_projection_gpu.test_projections_are_exact_under_the_exact_parity_build starts its child: with the exact-parity build of the kernels
    every int8 case of this file that is compared with a model or the oracle (sections 1, 2 and 4; section 3 compares the library with itself) passes with
    equality as its bar - projections and tm* included, normals and colours included, the march's controls against the
    oracle's bits"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(int8 or all_minimum) and not (exact_parity or range_skipping or update_volume)"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    cases = 4 * len(SC.ADDRESSING) + 5 * len(FRAME_ADDRESSING) + 4 * len(FRAME_ADDRESSING)      # sections 1, 2 and 4
    assert m and int(m.group(1)) == cases and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 3. range skipping is invisible, also behind ovr_hip_update_volume --------------------------------------------------------------------------------

def _families(ovr, iso, opacities):
    """name -> (case of a volume and camera, start(ren, case, skipping)): the frames whose skipping twins trust the macrocells' value ranges"""
    return {
        "maximum": (lambda vol, cam: TP._case(ovr, vol, cam=cam, rate=SC.FRAME_RATE), lambda ren, case, skip: TP._start(ovr, ren, case, MAXIMUM, skipping=skip)),
        "minimum": (lambda vol, cam: TP._case(ovr, vol, cam=cam, rate=SC.FRAME_RATE), lambda ren, case, skip: TP._start(ovr, ren, case, MINIMUM, skipping=skip)),
        "isosurface": (lambda vol, cam: TI._case(ovr, vol, cam=cam, rate=SC.FRAME_RATE, shading=2), lambda ren, case, skip: TI._start(ovr, ren, case, iso, skipping=skip)),
        "ao": (lambda vol, cam: TA._case(ovr, vol, cam=cam, rate=SC.FRAME_RATE, shading=1, size=SC.SIZE),
               lambda ren, case, skip: TA._start(ovr, ren, case, iso, opacities, ao=SC.AO, skipping=skip)),
    }


def _family_case(name, case_of, vol, cam):
    """the family's case under the oblique camera or the one behind the volume (isosurface_cases.BEHIND: its rays cross the slab volume's dim cells first)"""
    if cam == "behind" and name in ("maximum", "minimum"):
        return dict(case_of(vol, "axis"), cam=IC.BEHIND)
    if cam == "behind" and name == "ao":
        return case_of(vol, IC.BEHIND)
    return case_of(vol, cam)


def _conserved(a, b, name):
    """a: the plain frame, b: the skipping one - equal bits, every step either fetched or dropped"""
    assert TP._same(a[0], b[0]) and TP._same(a[1], b[1]), name
    sa, sb = a[2], b[2]
    assert sa.skipped_samples == 0 and sa.samples == sb.samples + sb.skipped_samples and sa.rays == sb.rays and sa.shaded_samples == sb.shaded_samples, name
    assert sa.skipped_shadow_samples == 0 and sa.shadow_samples == sb.shadow_samples + sb.skipped_shadow_samples, name


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", SC.SKIPPING_KINDS)
def test_range_skipping_is_invisible(ovr, hip_renderer_factory, monkeypatch, kind, dtype):
    SC.set_addressing(monkeypatch, None)
    vol = SC.volume(kind, dtype)
    iso = SC.scaled(IC.ISOVALUES[kind], dtype)
    ranges = ovr.projection.macrocell_ranges(vol)      # (the oracle's, bit for bit: tests/test_signed_types_model.py)
    skipped = {}
    for name, (case_of, start) in _families(ovr, iso, (0.4,) * (len(iso) - 1) + (1.0,)).items():
        for cam in ("oblique", "behind"):
            case = _family_case(name, case_of, vol, cam)
            plain, skipping = start(hip_renderer_factory(), case, False), start(hip_renderer_factory(), case, True)
            a, b = TP._render(ovr, plain), TP._render(ovr, skipping)
            _conserved(a, b, (kind, _name(dtype), name, cam))
            assert np.array_equal(TP._bits(skipping.macrocells()[0]), TP._bits(ranges)), (kind, _name(dtype), "the value ranges are not the model's")
            assert b[2].skipping_kernels == 1 and a[2].skipping_kernels == 0
            skipped[name] = skipped.get(name, 0) + b[2].skipped_samples + b[2].skipped_shadow_samples
            plain.close()
            skipping.close()
    print(f"{kind} {_name(dtype)}: steps skipped {skipped}")
    if kind == "slab":
        assert skipped["maximum"] > 0 and skipped["isosurface"] > 0, skipped


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", FRAME_ADDRESSING)
def test_update_volume_writes_the_minimum_across_a_cell_boundary(ovr, hip_renderer_factory, monkeypatch, am, dtype):
    """a box of the type's minimum (11 x 9 x 3 voxels across the macrocell borders x = 16 and y = 16) inside the dim cells behind the slab, whose ranges excluded the
    isovalue at 5 % of full scale: their minima move across it (macrocell_range_box_kernel of the signed types).  Second frames throughout - an AO frame's
    rotation follows the frame index.  The updated frame is a re-upload's bit for bit, counters and value ranges included, and the frame without skipping"""
    SC.set_addressing(monkeypatch, _am(am))
    dt = np.dtype(dtype)
    vol = SC.volume("slab", dtype)
    lowest = SC.MINIMUM[dt]
    patch = np.full((3, 9, 11), lowest, dt)
    lower = (14, 12, 15)
    patched = vol.copy()
    patched[lower[2]:lower[2] + 3, lower[1]:lower[1] + 9, lower[0]:lower[0] + 11] = patch
    iso = SC.scaled((0.05, 0.5), dtype)
    assert vol[15:].min() > (iso[0] * 127 if dt == np.int8 else iso[0]) > lowest
    for name, (case_of, start) in _families(ovr, iso, (0.4, 1.0)).items():
        case, case_new = _family_case(name, case_of, vol, "behind"), _family_case(name, case_of, patched, "behind")
        ren = start(hip_renderer_factory(), case, True)
        before = TP._render(ovr, ren)
        ren.update_volume(patch, lower)
        after = TP._render(ovr, ren)
        fresh_ren, plain_ren = start(hip_renderer_factory(), case_new, True), start(hip_renderer_factory(), case_new, False)
        fresh, plain = ([TP._render(ovr, r) for _ in range(2)][1] for r in (fresh_ren, plain_ren))
        tag = (_name(dtype), am, name)
        assert after[2].frame_index == fresh[2].frame_index == 2, tag
        assert TP._same(after[0], fresh[0]) and TP._same(after[1], fresh[1]) and _counters(after[2]) == _counters(fresh[2]), tag
        _conserved(plain, after, tag)
        assert np.array_equal(TP._bits(ren.macrocells()[0]), TP._bits(fresh_ren.macrocells()[0])), tag
        assert np.array_equal(TP._bits(ren.macrocells()[0]), TP._bits(ovr.projection.macrocell_ranges(patched))), (tag, "the updated value ranges are not the model's")
        if name != "maximum":      # (the maximum of a ray does not see a box of minima)
            assert not TP._same(after[1], before[1]) or not TP._same(after[0], before[0]), tag
        if name == "isosurface":
            assert before[2].skipped_samples > after[2].skipped_samples > 0, (tag, "the cells the box touched are fetched now")
        for r in (ren, fresh_ren, plain_ren):
            r.close()


# ---- 4. the march's controls on signed volumes -------------------------------------------------------------------------------------------------------

def clipped_march_body(ovr, oracle, make, dtype, check=True):
    """test_clipping_gpu.test_corner_cut_vs_oracle_crop, the dense table at rate 2 under full shading: the clipped frame is the oracle's frame of the crop"""
    lo, hi = (16, 16, 16), (32, 32, 32)
    case, crop = TC.crop_case(ovr, 32, dtype, lo, hi, "dense", "cut", 2.0, 2)
    out = []
    for pipeline in (1, 2):
        ren = make()
        rgba, grad, st = TC.render_clipped(ovr, ren, case, lo, hi, pipeline=pipeline)
        assert st.pipeline == pipeline
        ren.close()
        if check:
            ref, ref_grad, cnt = _once(("clip", _name(dtype)), lambda: TC.oracle_crop(oracle, case, crop, lo).render())
            assert cnt.samples > 0 and cnt.shaded_samples > 0
            TC.check_against_crop(oracle, f"clipped {_name(dtype)} pipeline {pipeline}", rgba, grad, st, ref, ref_grad, cnt)
        out.append((rgba, grad, _counters(st)))
    return out


def orthographic_march_body(ovr, oracle, make, dtype, check=True):
    """test_camera_gpu.test_march_vs_oracle_trace, the oblique camera under full shading: the frame is the oracle's march of the orthographic rays"""
    vol = ovr.synth.make_volume(24, dtype)
    case = TK._case(ovr, vol, CC.OBLIQUE, CC.BSIZE, shading=2)
    out = []
    for pipeline in (1, 2):
        ren = hip_setup(ovr, make(), case, pipeline=pipeline)
        TK._ortho(ovr, ren, CC.OBLIQUE, CC.BHEIGHT)
        for skip in (False, True):
            ren.set_empty_space_skipping(skip)
            ren.commit()
            rgba, grad, st = TK._render(ovr, ren)
            assert st.pipeline == pipeline
            if check:
                want, samples, hit = TK._trace(ovr, oracle, case, CC.BHEIGHT)
                assert 100 < hit.sum() < hit.size - 100
                name = (_name(dtype), pipeline, skip)
                compare(oracle, rgba, want, name=str(name))
                assert not rgba[~hit].any() and not grad[~hit].any(), name
                assert st.samples + st.skipped_samples == samples and st.rays == hit.size, name
            out.append((rgba, grad, (st.rays, st.samples + st.skipped_samples, st.shaded_samples, st.active_pixels)))
        ren.close()
    for f in out[1:]:
        assert TK._same(f[0], out[0][0])
    return out


def lit_march_body(ovr, oracle, make, dtype, check=True):
    """a light along (1, 1, 1) (test_lighting_gpu.test_light_direction_vs_oracle, the oracle's light set for the comparison) and half the reference material
    (test_half_material_is_half_the_frame_vs_oracle): twice the frame is the oracle's under that light"""
    case = TG._half_colour_case(ovr, oracle, tf="dense", cam="oblique", dtype=dtype)
    vec = [1.0, 1.0, 1.0]
    out = []
    for pipeline in (1, 2):
        ren = hip_setup(ovr, make(), case, pipeline=pipeline)
        ren.set_material(0.25, 0.25, 0.0, 0.0)
        ren.set_light_direction(vec, 1.0)
        ren.commit()
        ren.render()
        rgba, grad = hip_frame(ovr, ren)
        st = ren.stats()
        assert st.pipeline == pipeline and ren.lighting().is_reference == 0
        ren.close()
        if check:
            def reference():
                with TG.oracle_light(oracle, vec):
                    return oracle_scene(oracle, case).render()
            ref, _, cnt = _once(("lit", _name(dtype)), reference)
            doubled = rgba.copy()
            doubled[..., :3] *= F(2)   # exact
            assert ref[..., :3].max() > 0.05 and cnt.shadow_samples_visible > 0
            compare(oracle, doubled, ref, name=f"lit {_name(dtype)} pipeline {pipeline}")
            assert st.rays == cnt.rays and st.samples == cnt.samples and st.shaded_samples == cnt.shaded_samples
        out.append((rgba, grad, _counters(st)))
    return out


def cached_march_body(ovr, oracle, make, dtype, check=True):
    """test_shadow_cache_gpu: the built nodes against the oracle (nodes_vs_oracle), then a cached frame in each pipeline - the frame under the downloaded lattice,
    supplied (test_composition_identities)"""
    case = TS._case(ovr, oracle, dtype=dtype, tf="dense")
    if check:
        ren = make()
        TS.nodes_vs_oracle(ovr, oracle, ren, case, 4, f"nodes {_name(dtype)}")
        ren.close()
    out = []
    for pipeline in (1, 2):
        ren = TS._cached(ovr, make(), case, cell=4, pipeline=pipeline)
        built = TS._render(ovr, ren)
        lattice = ren.shadow_cache_values()
        assert ren.stats().pipeline == pipeline and ren.shadow_cache().builds == 1 and built[2][3] == 0 and built[2][2] > 0
        if check:
            ren.set_shadow_cache_values(lattice)
            ren.set_shadow_cache(TS.SUPPLIED)
            ren.commit()
            TS._same({"built": built, "supplied": TS._render(ovr, ren)})
        ren.close()
        out.append((built[0], built[1], built[2], lattice))
    TS._same({1: out[0][:3], 2: out[1][:3]})
    return out


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("am", FRAME_ADDRESSING)
@pytest.mark.parametrize("control", ("clip", "orthographic", "lit", "cached"))
def test_march_controls(ovr, oracle, hip_renderer_factory, monkeypatch, control, am, dtype):
    SC.set_addressing(monkeypatch, _am(am))
    body = {"clip": clipped_march_body, "orthographic": orthographic_march_body, "lit": lit_march_body, "cached": cached_march_body}[control]
    body(ovr, oracle, hip_renderer_factory, dtype)
