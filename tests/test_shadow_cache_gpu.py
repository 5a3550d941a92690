"""The shadow cache on the GPU (include/ovr_hip.h ovr_hip_set_shadow_cache).

The oracle pin: raymarching_shadow and the unshaded primary march are the same recurrence with another step, so the UNMODIFIED CPU oracle's
OracleScene(rate = r', shading = NONE).trace(org, light)[0][3] IS the shadow term at org of a renderer at rate r, provided 1 / r' equals the shadow stride
(1 / r * 10) * (1 / r) in float32 - the partner rate r' = float32(r * r / 10) does for r = 0.5, 1, 2, 3, 4 (asserted), and trace's sample counter is the
node's iteration count.  Under the exact-parity build (test_shadow_cache_is_exact_under_the_exact_parity_build starts this file that way) the built nodes
and the hook's values are the oracle's bits and the build's iteration counter is the sum of the oracle's counts; in the product they meet helpers.compare's
float bar (2e-4).  The lookup is fmaf alone: bit for bit against shadow_cache.py in both builds.  Everything else is identities between frames of the
renderer itself."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import EXACT_RUN, hip_frame, hip_setup, make_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETLIB = os.path.join(ROOT, "open-volume-renderer_amd", "libovr_hip_parity.so")
RENDERBATCH = os.path.join(ROOT, "oracle", "_ref", "renderbatch")
PLUGIN = os.path.join(ROOT, "plugin", "libdevice_hip.so")
F = np.float32
INF = float("inf")
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
SIZE = (48, 40)
MARCHED, CACHED, SUPPLIED = 0, 1, 2
TOL = 2e-4   # helpers.compare's float bar, the project's product bar
DTYPES = [np.float32, np.uint16, np.uint8]
ANISO = dict(n=0, dims=(40, 24, 20), spacing=(1.0, 1.5, 0.75), origin=(3.0, -2.0, 5.0), convention=1)


def _counters(st):
    return tuple(getattr(st, k) for k in COUNTERS)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _case(ovr, oracle, **kw):
    args = dict(n=32, tf="dense", cam="oblique", size=SIZE, shading=2)
    args.update(kw)
    return make_case(ovr, oracle, **args)


def _dims(case):
    nz, ny, nx = case["vol"].shape
    return (nx, ny, nz)


def _cached(ovr, ren, case, mode=CACHED, cell=4, **setup):
    hip_setup(ovr, ren, case, **setup)
    ren.set_shadow_cache(mode, cell)
    ren.commit()
    return ren


_oracle_scenes = {}


def oracle_shadow(ovr, oracle, case, light, pos, key=None):
    """the shadow term at world positions pos (n, 3) by the unmodified oracle: its unshaded primary march at the partner rate along the light -> (alpha, iterations)"""
    assert ovr.shadow_cache.partner_rate_exact(case["rate"])
    rp = float(ovr.shadow_cache.partner_rate(case["rate"]))
    w, h = case["size"]
    sc = _oracle_scenes.get(key) if key else None
    if sc is None:
        sc = oracle.OracleScene(case["vol"], case["colors"], case["alphas"], case["vr"], case["cam"], w, h, fovy=case["fovy"], rate=rp, shading=oracle.SHADE_NONE,
                                grid_origin=case["origin"], grid_spacing=case["spacing"], convention=case["convention"])
        if key:
            _oracle_scenes[key] = sc
    pos = np.asarray(pos, F).reshape(-1, 3)
    out, it = np.empty(len(pos), F), np.empty(len(pos), np.int64)
    for i, p in enumerate(pos):
        rgba, _, cnt = sc.trace(p, light)
        out[i], it[i] = rgba[3], cnt.samples
    return out, it


def check_values(name, got, want):
    d = float(np.abs(got - want).max())
    print(f"{name}: max |renderer - oracle| {d:.3g} over {got.size} values (mean {float(want.mean()):.3f}, {int((want > 0).sum())} > 0)")
    assert np.isfinite(got).all()
    if EXACT_RUN:
        assert _bits_equal(got, want), (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    else:
        assert d <= TOL, (name, d)


# ---- 1. the built nodes against the oracle -------------------------------------------------------------------------------------------------------

def nodes_vs_oracle(ovr, oracle, ren, case, cell, name, light=None):
    hip_setup(ovr, ren, case)
    if light is not None:
        ren.set_light_direction(light)
    ren.set_shadow_cache(CACHED, cell)
    ren.commit()
    values, pos = ren.shadow_cache_values(positions=True)
    sc = ren.shadow_cache()
    dims = _dims(case)
    n = ovr.shadow_cache.lattice_dims(dims, cell)
    assert (sc.mode, sc.cell, list(sc.dims), sc.valid, sc.builds) == (CACHED, cell, list(n), 1, 1) and sc.bytes == 4 * n[0] * n[1] * n[2]
    assert values.shape == (n[2], n[1], n[0])
    model = ovr.shadow_cache.node_positions(dims, cell, case["spacing"], case["origin"], vertex_centred=bool(case["convention"]))
    assert _bits_equal(pos, model), name
    unit = np.array(list(ren.lighting().direction), F)
    want, it = oracle_shadow(ovr, oracle, case, unit, model.reshape(-1, 3))
    assert 0 < (want > 0).sum() and want.min() >= 0 and want.max() <= 1 and (want < 0.9).sum() > 0
    check_values(name, values.ravel(), want)
    if EXACT_RUN:
        assert sc.build_shadow_samples == int(it.sum()), (name, sc.build_shadow_samples, int(it.sum()))
    print(f"{name}: build {sc.build_ms:.3f} ms, {sc.build_shadow_samples} iterations (oracle {int(it.sum())})")
    assert sc.build_shadow_samples > 0 and sc.build_ms > 0


@pytest.mark.parametrize("rate", [1.0, 2.0])
@pytest.mark.parametrize("tf", ["sparse", "dense"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_nodes_vs_oracle(ovr, oracle, hip_renderer_factory, dtype, tf, rate):
    case = _case(ovr, oracle, dtype=dtype, tf=tf, rate=rate)
    ren = hip_renderer_factory()
    nodes_vs_oracle(ovr, oracle, ren, case, 4, f"nodes {np.dtype(dtype).name} {tf} rate {rate}")
    ren.close()


def test_nodes_vs_oracle_second_light(ovr, oracle, hip_renderer_factory):
    case = _case(ovr, oracle, tf="sparse")
    ren = hip_renderer_factory()
    nodes_vs_oracle(ovr, oracle, ren, case, 2, "nodes, light (1, -0.5, 0.25), cell 2", light=(1.0, -0.5, 0.25))
    ren.close()


def test_nodes_vs_oracle_anisotropic_vertex_centred(ovr, oracle, hip_renderer_factory):
    """40 x 24 x 20 voxels, spacing (1, 1.5, 0.75), origin (3, -2, 5), cell 3 - no axis is a multiple of it: 15 x 9 x 8 nodes - vertex-centred"""
    case = _case(ovr, oracle, tf="dense", **ANISO)
    ren = hip_renderer_factory()
    nodes_vs_oracle(ovr, oracle, ren, case, 3, "nodes 40 x 24 x 20 vertex-centred cell 3")
    ren.close()


# ---- 2. the known-answer hook ---------------------------------------------------------------------------------------------------------------------

def _positions(rng, n, case):
    dims, spacing, origin = _dims(case), case["spacing"], case["origin"]
    ext = np.array(dims, np.float64) * np.array(spacing, np.float64)
    pos = np.array(origin) + (rng.random((n, 3)) * 1.5 - 0.25) * ext          # in and around the box
    pos[: n // 4] = np.array(origin) + rng.random((n // 4, 3)) * ext           # inside
    return pos.astype(F)


@pytest.mark.parametrize("which_case", ["cube", "aniso"])
def test_shadow_floats_march_vs_oracle(ovr, oracle, hip_renderer_factory, which_case):
    case = _case(ovr, oracle, tf="sparse", dtype=np.uint16) if which_case == "cube" else _case(ovr, oracle, tf="dense", rate=2.0, **ANISO)
    ren = hip_setup(ovr, hip_renderer_factory(), case)     # mode MARCHED: which = 0 works in every mode
    pos = _positions(np.random.default_rng(21), 2000, case)
    got = ren.shadow_floats(pos, 0)
    want, _ = oracle_shadow(ovr, oracle, case, np.array(list(ren.lighting().direction), F), pos)
    assert (want > 0).sum() > 50 and (want == 0).sum() > 0
    check_values(f"shadow_floats which 0, {which_case}", got, want)
    assert ren.shadow_cache().builds == 0
    with pytest.raises(RuntimeError, match="MARCHED"):
        ren.shadow_floats(pos, 1)
    ren.close()


@pytest.mark.parametrize("which_case", ["cube", "aniso"])
def test_shadow_floats_lookup_vs_model(ovr, oracle, hip_renderer_factory, which_case):
    """which = 1 against shadow_cache.lookup over the downloaded lattice: fmaf alone, bit for bit in both builds"""
    case = _case(ovr, oracle, tf="sparse") if which_case == "cube" else _case(ovr, oracle, tf="dense", **ANISO)
    cell = 2 if which_case == "cube" else 3
    ren = _cached(ovr, hip_renderer_factory(), case, cell=cell)
    lattice = ren.shadow_cache_values()
    assert lattice.max() > 0.1 and lattice.min() == 0
    pos = _positions(np.random.default_rng(22), 3000, case)
    nodes = ovr.shadow_cache.node_positions(_dims(case), cell, case["spacing"], case["origin"], vertex_centred=bool(case["convention"])).reshape(-1, 3)
    pos = np.concatenate([pos, nodes])
    inv, wp = ovr.clipping.volume_constants(_dims(case), case["spacing"], case["origin"], vertex_centred=bool(case["convention"]))
    want = ovr.shadow_cache.lookup(lattice, ovr.clipping.to_object(pos, inv, wp))
    got = ren.shadow_floats(pos, 1)
    assert _bits_equal(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert ren.shadow_cache().builds == 1
    # ... and the same lookup on a supplied lattice of other dimensions
    sup = np.random.default_rng(23).random((5, 7, 3)).astype(F)
    ren.set_shadow_cache_values(sup)
    ren.set_shadow_cache(SUPPLIED)
    ren.commit()
    assert _bits_equal(ren.shadow_floats(pos, 1), ovr.shadow_cache.lookup(sup, ovr.clipping.to_object(pos, inv, wp)))
    assert _bits_equal(ren.shadow_cache_values(), sup) and list(ren.shadow_cache().dims) == [3, 7, 5]
    ren.close()


def test_clipped_nodes_equal_the_hook_at_the_nodes(ovr, oracle, hip_renderer_factory):
    """with a clip box committed the clip is baked into the lattice: node == the shadow march from the node's position, bit for bit - and not the unclipped one"""
    case = _case(ovr, oracle, tf="dense", dtype=np.uint8)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.set_shadow_cache(CACHED, 4)
    ren.commit()
    plain = ren.shadow_cache_values()
    ren.set_clip_box((5.5, -INF, 9.0), (27.0, 20.25, INF))
    ren.commit()
    values, pos = ren.shadow_cache_values(positions=True)
    assert ren.shadow_cache().builds == 2
    assert _bits_equal(values.ravel(), ren.shadow_floats(pos.reshape(-1, 3), 0))
    assert np.abs(values - plain).max() > 0.05                                        # what is cut away casts no shadow: another lattice
    ren.close()


def test_shadow_cache_is_exact_under_the_exact_parity_build():
    """started the way tests/test_clipping_gpu.py starts its child: the exact-parity build of the kernels, the oracle in its "det" mode.  Items 1 and 2: the nodes
    and the hook's values are the oracle's bits, build_shadow_samples is the sum of the oracle's counts"""
    assert os.path.exists(DETLIB), "libovr_hip_parity.so is missing: make -C open-volume-renderer_amd/csrc parity (build() does)"
    env = dict(os.environ, OVR_HIP_LIBRARY=DETLIB, OVR_PARITY_EXACT_RUN="1", OVR_ORACLE_POWF="det")
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "nodes_vs_oracle or shadow_floats or clipped_nodes"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = out.stdout[-2500:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) >= 12 + 2 + 4 + 1 and "failed" not in out.stdout.splitlines()[-1], tail


# ---- 3. composition identities --------------------------------------------------------------------------------------------------------------------

def _render(ovr, ren):
    ren.render()
    st = ren.stats()
    return hip_frame(ovr, ren) + (_counters(st),)


def _same(frames):
    base = next(iter(frames.values()))
    for k, (rgba, grad, cnt) in frames.items():
        assert _bits_equal(rgba, base[0]) and _bits_equal(grad, base[1]), k
        assert cnt == base[2], (k, cnt, base[2])
    return base


@pytest.mark.parametrize("pipeline", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_composition_identities(ovr, oracle, hip_renderer_factory, dtype, pipeline):
    case = _case(ovr, oracle, tf="bumps", dtype=dtype)
    ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
    ren.set_shading(1)
    ren.commit()
    gradient = _render(ovr, ren)
    ren.set_material(0.5, 0.0, 0.0, 0.0)
    ren.commit()
    ambient = _render(ovr, ren)
    assert ren.stats().pipeline == pipeline and gradient[2][2] > 0 and not np.array_equal(gradient[0], ambient[0])
    ren.set_material()
    ren.set_shading(2)
    n = (7, 5, 6)
    # all zeros: no shadow anywhere == the gradient-shaded frame
    ren.set_shadow_cache_values(np.zeros((n[2], n[1], n[0]), F))
    ren.set_shadow_cache(SUPPLIED)
    ren.commit()
    zeros = _render(ovr, ren)
    _same({"gradient": gradient, "supplied zeros": zeros})
    assert ren.stats().pipeline == pipeline and zeros[2][3] == 0 and zeros[2][6] == 0
    # all ones: everything in shadow == ambient alone (zero-gradient samples are NaN on both sides, and clamp01 takes both to 0)
    ren.set_shadow_cache_values(np.ones((n[2], n[1], n[0]), F))
    ren.commit()
    ones = _render(ovr, ren)
    _same({"ambient": ambient, "supplied ones": ones})
    # a built lattice, downloaded and supplied: the same frame
    ren.set_shadow_cache(CACHED, 4)
    ren.commit()
    built = _render(ovr, ren)
    lattice = ren.shadow_cache_values()
    assert ren.shadow_cache().builds == 1 and built[2][3] == 0 and not np.array_equal(built[0], zeros[0]) and not np.array_equal(built[0], ones[0])
    ren.set_shadow_cache_values(lattice)
    ren.set_shadow_cache(SUPPLIED)
    ren.commit()
    _same({"built": built, "supplied": _render(ovr, ren)})
    assert ren.shadow_cache().builds == 1
    ren.close()


# ---- 4. invariants of one cached frame --------------------------------------------------------------------------------------------------------------

def test_invariant_pipelines_skipping_layouts(ovr, oracle, hip_renderer_factory):
    case = _case(ovr, oracle, tf="bumps")
    frames = {}
    for pipeline in (1, 2):
        for skip in (False, True):
            for layout in (0, 1, 2, 3):
                if layout and (pipeline, skip) not in ((1, False), (2, True)):
                    continue
                ren = hip_renderer_factory()
                ren.set_volume_layouts(2)
                ren.set_layout_choice(layout)
                hip_setup(ovr, ren, case, pipeline=pipeline)
                ren.set_empty_space_skipping(skip)
                ren.set_shadow_cache(CACHED, 2)
                ren.commit()
                ren.render()
                st = ren.stats()
                assert st.layout == layout and st.pipeline == pipeline and st.shadow_samples == 0 and st.skipped_shadow_samples == 0
                frames[(pipeline, skip, layout)] = hip_frame(ovr, ren) + ((st.rays, st.samples + st.skipped_samples, st.shaded_samples),)
                assert ren.shadow_cache().builds == 1
                ren.close()
    base = _same(frames)
    assert base[0][..., :3].max() > 0.1 and base[2][2] > 0


def test_invariant_device_group_and_image_shards(ovr, oracle, hip_renderer_factory):
    case = _case(ovr, oracle, tf="sparse", size=(49, 37))
    single = _cached(ovr, hip_renderer_factory(), case, cell=2)
    want = _render(ovr, single)
    lattice = single.shadow_cache_values()
    group = ovr.create_renderer("hip", devices=[0, 0, 0])
    try:
        _cached(ovr, group, case, cell=2)
        got = _render(ovr, group)
        for member in range(3):          # every member builds its own, identical lattice
            assert _bits_equal(group.shadow_cache_values(member), lattice), member
        assert group.shadow_cache().builds == 1
    finally:
        group.close()
    _same({"single": want, "group of 3": got})
    # image shards: every rank builds the whole lattice (view-independent; redundant across ranks) and its tiles are the full frame's
    w, h = case["size"]
    ty, tx = np.mgrid[0:h, 0:w]
    for rank in range(2):
        ren = hip_setup(ovr, hip_renderer_factory(), case)
        ren.set_image_shard(rank, 2, 16, 16)
        ren.set_shadow_cache(CACHED, 2)
        ren.commit()
        ren.render()
        rgba, grad = hip_frame(ovr, ren)
        own = ((tx // 16 + ty // 16) % 2) == rank
        assert _bits_equal(rgba[own], want[0][own]) and _bits_equal(grad[own], want[1][own]) and _bits_equal(ren.shadow_cache_values(), lattice)
        ren.close()
    single.close()


def test_invariant_accumulation_spp2(ovr, oracle, hip_renderer_factory):
    case = _case(ovr, oracle, tf="dense", spp=2)
    frames = {}
    for pipeline in (1, 2):
        ren = _cached(ovr, hip_renderer_factory(), case, cell=4, accumulate=True, pipeline=pipeline)
        for _ in range(3):
            out = _render(ovr, ren)
        assert ren.stats().frame_index == 3 and ren.shadow_cache().builds == 1
        frames[pipeline] = out
        ren.close()
    _same(frames)


# ---- 5. staleness and the neutral element ----------------------------------------------------------------------------------------------------------

def test_staleness(ovr, oracle, hip_renderer_factory):
    case = _case(ovr, oracle, tf="dense", dtype=np.uint16)
    ren = _cached(ovr, hip_renderer_factory(), case, cell=4, accumulate=True)
    ren.render()
    assert ren.shadow_cache().builds == 1 and ren.shadow_cache().valid == 1
    # what does not touch the lattice
    eye, at, up = case["cam"]
    neutral = [lambda: ren.set_camera((eye[0] + 3.0, eye[1], eye[2]), at, up), lambda: ren.set_fbsize((40, 32)), lambda: ren.set_material(0.3, 0.7, 0.2, 10.0),
               lambda: ren.set_light_direction(None, 1.5), lambda: ren.set_sample_per_pixel(2), lambda: ren.set_shading_pipeline(2), lambda: ren.set_empty_space_skipping(True),
               lambda: ren.set_frame_accumulation(False), lambda: ren.set_shadow_cache(CACHED, 4)]
    for i, change in enumerate(neutral):
        change()
        ren.commit()
        ren.render()
        sc = ren.shadow_cache()
        assert sc.builds == 1 and sc.valid == 1, i
        assert ren.stats().shadow_samples == 0
    ren.set_sample_per_pixel(1); ren.set_frame_accumulation(True); ren.set_light_direction(None, 1.0); ren.set_material()
    ren.commit()
    # what does: each raises builds by one, and the lattice afterwards is a fresh renderer's
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.uint16)
    patch = np.full((6, 5, 7), 40000, np.uint16)
    state = dict(tf="dense", rate=1.0, light=None, clip=None, convention=0, cell=4, patch=False)

    def fresh():
        c = _case(ovr, oracle, tf=state["tf"], dtype=np.uint16, rate=state["rate"], convention=state["convention"])
        c = dict(c, cam=case["cam"])
        other = hip_setup(ovr, hip_renderer_factory(), c)
        if state["patch"]:
            other.update_volume(patch, (9, 11, 13))
        if state["light"]:
            other.set_light_direction(state["light"])
        if state["clip"]:
            other.set_clip_box(*state["clip"])
        other.set_shadow_cache(CACHED, state["cell"])
        other.commit()
        v = other.shadow_cache_values()
        other.close()
        return v

    changes = [("transfer function", lambda: (ren.set_transfer_function(colors, alphas, vr), state.update(tf="sparse"))),
               ("sampling rate", lambda: (ren.set_volume_sampling_rate(2.0), state.update(rate=2.0))),
               ("light direction", lambda: (ren.set_light_direction((0.3, 1.0, 0.2)), state.update(light=(0.3, 1.0, 0.2)))),
               ("clip box", lambda: (ren.set_clip_box((4.0, 0.0, 0.0), (32.0, 28.0, 32.0)), state.update(clip=((4.0, 0.0, 0.0), (32.0, 28.0, 32.0))))),
               ("grid convention", lambda: (ren.set_grid_convention(1), state.update(convention=1))),
               ("cell", lambda: (ren.set_shadow_cache(CACHED, 3), state.update(cell=3))),
               ("update_volume", lambda: (ren.update_volume(patch, (9, 11, 13)), state.update(patch=True)))]
    builds = 1
    for name, change in changes:
        change()
        ren.commit()
        assert ren.shadow_cache().valid == 0, name
        ren.render()
        builds += 1
        sc = ren.shadow_cache()
        assert sc.builds == builds and sc.valid == 1, (name, sc.builds, builds)
        assert ren.stats().frame_index == 1, name
        assert _bits_equal(ren.shadow_cache_values(), fresh()), name
        ren.render()
        assert ren.shadow_cache().builds == builds and ren.stats().frame_index == 2, name
    ren.close()


@pytest.mark.parametrize("pipeline", [1, 2])
def test_marched_mode_and_other_shadings_are_untouched(ovr, oracle, hip_renderer_factory, pipeline):
    case = _case(ovr, oracle, tf="bumps")
    never = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
    want = {2: _render(ovr, never)}
    for shading in (0, 1):
        never.set_shading(shading); never.commit()
        want[shading] = _render(ovr, never)
    never.close()
    assert want[2][2][3] > 0
    ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
    ren.set_shadow_cache(CACHED, 2); ren.commit(); ren.render()
    assert ren.shadow_cache().builds == 1 and ren.stats().shadow_samples == 0
    ren.set_shadow_cache(MARCHED); ren.commit()
    sc = ren.shadow_cache()
    assert (sc.mode, sc.valid, sc.bytes, list(sc.dims)) == (MARCHED, 0, 0, [0, 0, 0])
    _same({"never": want[2], "marched again": _render(ovr, ren)})
    ren.close()
    for shading in (0, 1):
        ren = hip_setup(ovr, hip_renderer_factory(), case, pipeline=pipeline)
        ren.set_shading(shading)
        ren.set_shadow_cache(CACHED, 2)
        ren.commit()
        _same({"never": want[shading], "cached, not full": _render(ovr, ren)})
        assert ren.shadow_cache().builds == 0
        ren.close()


# ---- 6. ordering on frames ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tf", ["dense", "sparse"])
def test_cached_frame_is_closer_to_the_marched_one_than_no_shadows(ovr, oracle, hip_renderer_factory, tf):
    case = _case(ovr, oracle, tf=tf)
    ren = hip_setup(ovr, hip_renderer_factory(), case)
    ren.render()
    marched = oracle.rgba8(hip_frame(ovr, ren)[0]).astype(int)
    assert ren.stats().shadow_samples > 0
    ren.set_shadow_cache(CACHED, 2); ren.commit(); ren.render()
    cached = oracle.rgba8(hip_frame(ovr, ren)[0]).astype(int)
    ren.set_shadow_cache(MARCHED); ren.set_shading(1); ren.commit(); ren.render()
    gradient = oracle.rgba8(hip_frame(ovr, ren)[0]).astype(int)
    ren.close()
    e_cached, e_none = float(np.abs(cached - marched).mean()), float(np.abs(gradient - marched).mean())
    print(f"{tf}: mean |cached - marched| {e_cached:.3f}, mean |gradient only - marched| {e_none:.3f} (8-bit)")
    assert e_none > 0 and e_cached < e_none


# ---- 7. error codes and state rules ---------------------------------------------------------------------------------------------------------------

def test_error_codes_and_state(ovr, oracle, hip_renderer_factory):
    case = _case(ovr, oracle, tf="dense")
    L = ovr._lib
    lib = L.load()
    ren = hip_setup(ovr, hip_renderer_factory(), case, accumulate=True)
    h = ren._h
    sc = ren.shadow_cache()
    assert (sc.mode, sc.cell, list(sc.dims), sc.valid, sc.builds, sc.bytes) == (MARCHED, 4, [0, 0, 0], 0, 0, 0)
    ren.render(); ren.render()
    assert lib.ovr_hip_set_shadow_cache(h, 3, 4) == -1 and b"ovr_hip_set_shadow_cache" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_set_shadow_cache(h, -1, 4) == -1
    assert lib.ovr_hip_set_shadow_cache(h, CACHED, -1) == -1
    assert lib.ovr_hip_set_shadow_cache(h, SUPPLIED, 0) == -3 and b"values" in lib.ovr_hip_last_error()     # ESTATE: nothing uploaded
    i3 = lambda v: (L.C.c_int32 * 3)(*v)
    ok = np.zeros(8, F)
    fp = lambda a: a.ctypes.data
    assert lib.ovr_hip_set_shadow_cache_values(h, None, 0, i3((2, 2, 2))) == -1
    assert lib.ovr_hip_set_shadow_cache_values(h, fp(ok), 0, i3((2, 1, 4))) == -1
    assert lib.ovr_hip_set_shadow_cache_values(h, fp(ok), 7, i3((2, 2, 2))) == -1
    assert lib.ovr_hip_set_shadow_cache_values(h, fp(ok), 0, i3((2048, 2048, 2048))) == -1 and b"2^31" in lib.ovr_hip_last_error()
    for bad in (np.nan, np.inf):
        v = ok.copy(); v[5] = bad
        assert lib.ovr_hip_set_shadow_cache_values(h, fp(v), 0, i3((2, 2, 2))) == -1 and b"finite" in lib.ovr_hip_last_error()
    assert lib.ovr_hip_set_shadow_cache(h, SUPPLIED, 0) == -3                                                  # still nothing uploaded
    ren.commit(); ren.render()                                                                                 # nothing was queued by the refused calls
    assert ren.stats().frame_index == 3 and ren.shadow_cache().mode == MARCHED
    with pytest.raises(RuntimeError, match="MARCHED"):
        ren.shadow_cache_values()
    # queued: nothing happens before the commit, the getter reports the committed state; cell 0 is the default 4
    ren.set_shadow_cache(CACHED, 0)
    ren.render()
    assert ren.stats().frame_index == 4 and ren.shadow_cache().mode == MARCHED and ren.stats().shadow_samples > 0
    ren.commit(); ren.render()
    sc = ren.shadow_cache()
    assert ren.stats().frame_index == 1 and (sc.mode, sc.cell, list(sc.dims), sc.builds) == (CACHED, 4, [9, 9, 9], 1)
    ren.set_shadow_cache(CACHED, 4); ren.commit(); ren.render()          # the same value again resets nothing
    assert ren.stats().frame_index == 2 and ren.shadow_cache().builds == 1
    ren.set_shadow_cache(CACHED, 2); ren.commit(); ren.render()          # another cell does
    assert ren.stats().frame_index == 1 and list(ren.shadow_cache().dims) == [17, 17, 17] and ren.shadow_cache().builds == 2
    # a lattice of more than 2^31 - 1 nodes for the resident volume: 32^3 voxels cannot get there, the node rule can (policy: ceil(dim / cell) + 1 per axis)
    # supplied values survive until the mode leaves SUPPLIED
    ren.set_shadow_cache_values(np.full((2, 2, 2), 0.25, F))
    ren.set_shadow_cache(SUPPLIED); ren.commit(); ren.render()
    assert ren.shadow_cache().mode == SUPPLIED and list(ren.shadow_cache().dims) == [2, 2, 2] and ren.shadow_cache().valid == 1 and ren.shadow_cache().builds == 2
    ren.set_shadow_cache(CACHED, 2); ren.commit()
    assert lib.ovr_hip_set_shadow_cache(h, SUPPLIED, 0) == -3            # the values went with the mode
    ren.render()
    assert ren.shadow_cache().builds == 3
    ren.close()


def test_a_mode_change_voids_the_tuners_measurement(ovr, oracle, hip_renderer_factory):
    """as tests/test_clipping_gpu.py::test_a_box_change_voids_the_tuners_measurement: a cached frame is another workload"""
    case = make_case(ovr, oracle, n=48, tf="dense", cam="front", size=(96, 64), shading=2, rate=2.0)
    ren = hip_renderer_factory()
    ren.set_volume_layouts(2)
    hip_setup(ovr, ren, case)
    seen = []
    for _ in range(14):
        ren.render()
        seen.append(ren.stats().tuning)
    assert seen[-1] == 2 and 1 in seen, seen
    ren.set_shadow_cache(CACHED, 4)
    ren.commit()
    ren.render()
    assert ren.stats().tuning == 0 and ren.stats().shadow_samples == 0
    ren.close()


# ---- 8. the drop-in plugin ------------------------------------------------------------------------------------------------------------------------

def test_renderbatch_shadow_cache_variable(tmp_path, ovr, oracle, hip_renderer_factory):
    if not (os.path.exists(RENDERBATCH) and os.path.exists(PLUGIN)):
        pytest.skip("oracle/_ref/renderbatch or plugin/libdevice_hip.so missing: they are built by __graft_entry__.build() where the reference tree is present and travel with the snapshot")
    from PIL import Image
    n, W, H = 40, 96, 64
    vol = ovr.synth.make_volume(n, np.float32)
    colors, alphas, vr = ovr.synth.make_tfn("dense", 256, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    scene_path = ovr.vidi3d.write_scene(str(tmp_path), "synthetic", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), cam, fovy=45.0, sample_distance=0.25)
    env0 = dict(os.environ)
    env0["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(PLUGIN), os.path.join(ROOT, "open-volume-renderer_amd"), env0.get("LD_LIBRARY_PATH", "")])
    for k in ("OVR_HIP_SHADOW_CACHE", "OVR_HIP_QUIET"):
        env0.pop(k, None)

    def batch(tag, **extra):
        out = subprocess.run([RENDERBATCH, "--scene", scene_path, "--num-frames", "1", "--device", "hip", "--fbsize", f"{W},{H}", "--exp", str(tmp_path / tag)],
                             env=dict(env0, **extra), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        return np.asarray(Image.open(str(tmp_path / f"{tag}000000.png")).convert("RGBA")), out.stderr

    plain, err = batch("plain")
    assert "[hip] shadow cache" not in err
    cached, err = batch("cached", OVR_HIP_SHADOW_CACHE="2")
    assert "[hip] shadow cache: one node per 2 voxels" in err

    def host(cell):
        scene, camera = ovr.vidi3d.scene_from_file(scene_path)
        ren = hip_renderer_factory()
        ren.set_fbsize((W, H))
        ren.set_frame_accumulation(True)
        ren.set_volume_sampling_rate(1.0)        # main_batch.cpp:69
        ren.init(scene, camera)
        ren.set_camera(camera.eye, camera.at, camera.up)   # fovy 60 (renderer.h:149-152)
        if cell:
            ren.set_shadow_cache(CACHED, cell)
        ren.commit()
        ren.render()
        assert (ren.stats().shadow_samples == 0) == bool(cell)
        return oracle.rgba8(hip_frame(ovr, ren)[0], flip=True).reshape(H, W, 4)

    want_plain, want_cached = host(0), host(2)
    assert np.abs(plain.astype(int) - want_plain.astype(int)).max() <= 1
    assert np.abs(cached.astype(int) - want_cached.astype(int)).max() <= 1
    assert np.abs(want_cached.astype(int) - want_plain.astype(int)).max() > 0
