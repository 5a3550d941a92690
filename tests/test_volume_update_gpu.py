"""ovr_hip_update_volume on the GPU (include/ovr_hip.h).  The definition is an equivalence and needs no tolerance: after an update
every observable of the renderer - the raw bytes of every resident layout, the macrocell grids, ovr_hip_get_volume_info, frames, gradient layer and counters
under every forced layout, both pipelines, with and without empty-space skipping - is bit for bit what a fresh renderer shows that was set with the patched
array.  Fresh layouts are poisoned (OVR_HIP_POISON_ALLOC): an element an update must not touch, or a fresh upload forgets, shows.

Volumes: 70 x 67 x 69 - more than two macro blocks on every axis in every layout (30, 28 and 32 cells wide), no dimension a multiple of a brick - and
3 x 2 x 5, smaller than one brick."""
import ctypes as C

import numpy as np
import pytest

from helpers import compare, hip_frame, hip_setup, oracle_scene

pytestmark = pytest.mark.gpu
F = np.float32
COUNTERS = ("rays", "samples", "shaded_samples", "shadow_samples", "active_pixels", "skipped_samples", "skipped_shadow_samples")
BIG, SMALL = (70, 67, 69), (3, 2, 5)
EINVAL, ESTATE = -1, -3   # include/ovr_hip.h
SIZE = (48, 40)


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("OVR_HIP_POISON_ALLOC", "1")


@pytest.fixture
def made(ovr):
    rs = []

    def make(devices=None):
        r = ovr.create_renderer("hip", devices=devices) if devices else ovr.create_renderer("hip")
        rs.append(r)
        return r

    yield make
    for r in rs:
        r.close()


_base = {}


def base_volume(ovr, dtype, dims):
    """the synthetic field on dims = (nx, ny, nz), computed once per type and shared read-only"""
    key = (np.dtype(dtype).name, dims)
    if key not in _base:
        v = ovr.synth.make_volume(0, dtype, dims=dims)
        v.setflags(write=False)
        _base[key] = v
    return _base[key]


def make_case(ovr, vol, tf="sparse", cam="oblique", size=SIZE, shading=2, vr=None):
    colors, alphas, r = ovr.synth.make_tfn(tf, 256, vol.dtype)
    return dict(vol=vol, colors=colors, alphas=alphas, vr=r if vr is None else vr, cam=ovr.synth.make_camera(cam, max(vol.shape)), size=size, shading=shading,
                rate=1.0, spp=1, convention=0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=60.0)


def setup(ovr, ren, case, vol, layouts=2, accumulate=False):
    ren.set_volume_layouts(layouts)
    return hip_setup(ovr, ren, dict(case, vol=vol), accumulate=accumulate)


def patch_values(rng, v0, shape, lo=None, hi=None):
    """random voxels from V0's own range (or [lo, hi]) in V0's type"""
    lo = float(v0.min()) if lo is None else lo
    hi = float(v0.max()) if hi is None else hi
    p = rng.uniform(lo, hi, shape)
    return (np.rint(p) if v0.dtype.kind in "iu" else p).astype(v0.dtype)


def patched(v0, patch, lower):
    x, y, z = lower
    v1 = v0.copy()
    v1[z:z + patch.shape[0], y:y + patch.shape[1], x:x + patch.shape[2]] = patch
    return v1


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def layouts_of(ren, member=0):
    """the bytes of layouts 0 ... 3, None where the type has no such replica"""
    out = []
    for k in range(4):
        try:
            out.append(ren.volume_layout(k, member))
        except RuntimeError as e:
            assert "not resident" in str(e), e
            out.append(None)
    return out


def assert_same_layouts(a, b, what=""):
    la, lb = layouts_of(a), layouts_of(b)
    assert la[0] is not None
    for k in range(4):
        assert (la[k] is None) == (lb[k] is None), (what, k)
        if la[k] is not None:
            assert la[k].size == lb[k].size and np.array_equal(la[k], lb[k]), f"{what}: layout {k}: {int((la[k] != lb[k]).sum())} of {la[k].size} bytes differ"


def info_tuple(ren):
    v = ren.volume_info()
    return (tuple(v.dims), v.value_type, v.resident_bytes) + tuple(bits([v.data_lower, v.data_upper, v.tf_lower, v.tf_upper]))


def observe(ovr, ren):
    ren.render()
    rgba, grad = hip_frame(ovr, ren)
    st = ren.stats()
    return bits(rgba), bits(grad), tuple(getattr(st, k) for k in COUNTERS)


def assert_same_frames(ovr, a, b, what="", layouts=(0, 1, 2, 3), pipelines=(1, 2), skipping=(False, True)):
    for layout in layouts:
        for pipe in pipelines:
            for skip in skipping:
                got = []
                for ren in (a, b):
                    ren.set_layout_choice(layout)
                    ren.set_shading_pipeline(pipe)
                    ren.set_empty_space_skipping(skip)
                    ren.commit()
                    got.append(observe(ovr, ren))
                (ra, ga, ca), (rb, gb, cb) = got
                tag = f"{what}: layout {layout} pipeline {pipe} skipping {skip}"
                assert ca == cb, (tag, ca, cb)
                assert np.array_equal(ra, rb), f"{tag}: {int((ra != rb).sum())} frame words differ"
                assert np.array_equal(ga, gb), f"{tag}: {int((ga != gb).sum())} gradient words differ"
                assert ca[1] > 0, tag


def assert_equivalent(ovr, a, b, what=""):
    assert_same_layouts(a, b, what)
    (mma, mja), (mmb, mjb) = a.macrocells(), b.macrocells()
    assert np.array_equal(bits(mma), bits(mmb)), f"{what}: macrocell ranges: cells {np.argwhere((bits(mma) != bits(mmb)).any(axis=-1))[:8].tolist()}"
    assert np.array_equal(bits(mja), bits(mjb)), f"{what}: majorants"
    assert info_tuple(a) == info_tuple(b), (what, info_tuple(a), info_tuple(b))
    assert_same_frames(ovr, a, b, what)
    assert_same_layouts(a, b, what + " (after the frames)")


def update_vs_fresh(ovr, made, v0, patch, lower, tf="sparse"):
    """renderer A: set with V0, rendered, updated, rendered; renderer B: set fresh with V1"""
    v1 = patched(v0, patch, lower)
    case = make_case(ovr, v0, tf=tf)
    a = setup(ovr, made(), case, v0)
    a.render()
    a.update_volume(patch, lower)
    a.render()
    b = setup(ovr, made(), case, v1)
    b.render()
    assert_equivalent(ovr, a, b, f"{v0.dtype.name} box {tuple(lower)} + {patch.shape[::-1]}")
    return a, b


# ---- 1. update = re-upload ----------------------------------------------------------------------------------------------------------------------------------

# (lower, extent) in (x, y, z) on the 70 x 67 x 69 volume
BOXES = {
    "one_voxel": ((33, 30, 37), (1, 1, 1)),
    "interior": ((24, 31, 17), (20, 9, 13)),
    "face_x0": ((0, 20, 20), (5, 30, 9)),
    "face_x1": ((61, 5, 40), (9, 11, 20)),
    "face_y0": ((10, 0, 3), (33, 2, 29)),
    "face_y1": ((29, 63, 30), (31, 4, 5)),
    "face_z0": ((40, 40, 0), (17, 16, 3)),
    "face_z1": ((2, 3, 64), (60, 30, 5)),
    "corner": ((66, 64, 65), (4, 3, 4)),
    "whole": ((0, 0, 0), BIG),
}
DTYPES = [np.float32, np.uint16, np.uint8, np.int16]


@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_update_equals_reupload(ovr, made, dtype, name):
    lower, extent = BOXES[name]
    v0 = base_volume(ovr, dtype, BIG)
    patch = patch_values(np.random.default_rng(11), v0, extent[::-1])
    update_vs_fresh(ovr, made, v0, patch, lower)


@pytest.mark.parametrize("name,lower,extent", [("one_voxel", (1, 1, 2), (1, 1, 1)), ("corner", (2, 1, 4), (1, 1, 1)), ("face", (0, 0, 1), (3, 1, 2)), ("whole", (0, 0, 0), SMALL)])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_update_equals_reupload_smaller_than_a_brick(ovr, made, dtype, name, lower, extent):
    v0 = base_volume(ovr, dtype, SMALL)
    lo, hi = {"f": (0.0, 1.0), "u": (0.0, float(np.iinfo(dtype).max) if np.dtype(dtype).kind == "u" else 0.0), "i": (-30000.0, 30000.0)}[np.dtype(dtype).kind]
    patch = patch_values(np.random.default_rng(12), v0, extent[::-1], lo, hi)
    update_vs_fresh(ovr, made, v0, patch, lower, tf="dense")


def peaked(v0):
    """V0 with ONE voxel above everything else, and where it is (x, y, z)"""
    top = {"f": 2.0, "u": float(np.iinfo(v0.dtype).max) if v0.dtype.kind == "u" else 0.0, "i": 32767.0}[v0.dtype.kind]
    v = v0.copy()
    if v0.dtype.kind in "iu":
        v = np.minimum(v, v0.dtype.type(top - 1))
    p = (41, 29, 50)
    v[p[2], p[1], p[0]] = top
    assert (v == v.max()).sum() == 1
    return v, p, top


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_box_that_raises_the_data_range(ovr, made, dtype):
    v0 = base_volume(ovr, dtype, BIG)
    _, _, top = peaked(v0)
    v0 = np.minimum(v0, v0.dtype.type(top - 1)) if v0.dtype.kind in "iu" else v0
    patch = patch_values(np.random.default_rng(13), v0, (5, 6, 7))
    patch[2, 3, 4] = top
    a, _ = update_vs_fresh(ovr, made, v0, patch, (30, 20, 10))
    assert a.volume_info().data_upper > float(v0.max()) / (255.0 if dtype == np.uint8 else 1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_box_that_removes_the_maximum(ovr, made, dtype):
    base = base_volume(ovr, dtype, BIG)
    v0, p, top = peaked(base)
    lower = (p[0] - 2, p[1] - 1, p[2] - 3)
    patch = np.ascontiguousarray(base[lower[2]:lower[2] + 6, lower[1]:lower[1] + 3, lower[0]:lower[0] + 5])
    patch = np.minimum(patch, v0.dtype.type(top - 1)) if v0.dtype.kind in "iu" else patch
    a, _ = update_vs_fresh(ovr, made, v0, patch, lower)
    assert a.volume_info().data_upper < top / (255.0 if dtype == np.uint8 else 1.0)


@pytest.mark.parametrize("dtype", [np.float64, np.uint32, np.int32], ids=lambda d: np.dtype(d).name)
def test_update_converts_like_the_upload(ovr, made, dtype):
    v0 = base_volume(ovr, dtype, BIG)
    info = None if np.dtype(dtype).kind == "f" else np.iinfo(dtype)
    patch = patch_values(np.random.default_rng(14), v0, (13, 9, 20), *((0.0, 1.0) if info is None else (float(info.min), float(info.max))))
    update_vs_fresh(ovr, made, v0, patch, (24, 31, 17))


# ---- 2. oracle ----------------------------------------------------------------------------------------------------------------------------------------------

def test_an_updated_frame_meets_the_oracle(ovr, oracle, made):
    v0 = base_volume(ovr, np.float32, BIG)
    patch = patch_values(np.random.default_rng(15), v0, (30, 28, 26))
    lower = (20, 18, 22)
    v1 = patched(v0, patch, lower)
    case = make_case(ovr, v0, tf="sparse", size=(64, 48), shading=2)
    ren = setup(ovr, made(), case, v0)
    ren.render()
    before = hip_frame(ovr, ren)[0]
    ren.update_volume(patch, lower)
    ren.render()
    rgba = hip_frame(ovr, ren)[0]
    assert not np.array_equal(bits(before), bits(rgba))
    ref, _, cnt = oracle_scene(oracle, dict(case, vol=v1)).render()
    compare(oracle, rgba, ref, name="updated frame")
    assert ren.stats().samples == cnt.samples


# ---- 3. background replicas ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", ["front", "oblique"])
def test_an_update_right_behind_a_background_build(ovr, made, cam):
    """layouts mode 1: the first frame with automatic layout choice starts a replica's build on a builder thread; the update follows at once.  Whichever
    way the race goes - the build reads the general layout before the update writes it and is patched, or is enqueued behind it - every layout ends up
    as a fresh renderer's"""
    v0 = base_volume(ovr, np.float32, BIG)
    patch = patch_values(np.random.default_rng(16), v0, (13, 9, 20))
    lower = (24, 31, 17)
    case = make_case(ovr, v0, tf="dense", cam=cam)
    a = setup(ovr, made(), case, v0, layouts=1)
    a.set_layout_choice(-1)
    a.commit()
    a.render()
    a.update_volume(patch, lower)
    b = setup(ovr, made(), case, patched(v0, patch, lower), layouts=1)
    assert_same_frames(ovr, a, b, cam, pipelines=(2,), skipping=(False,))   # forces every layout: each replica is built or waited for
    assert_same_layouts(a, b, cam)
    assert all(l is not None for l in layouts_of(a))


# ---- 4. state -----------------------------------------------------------------------------------------------------------------------------------------------

def test_accumulation_and_retired_blocks_start_over(ovr, made):
    v0 = base_volume(ovr, np.float32, BIG)
    case = make_case(ovr, v0)
    ren = setup(ovr, made(), case, v0, accumulate=True)
    ren.set_convergence(2, 0.0)   # adaptive, threshold 0: a static scene retires every block after frame 2
    ren.commit()
    for _ in range(3):
        ren.render()
    c = ren.convergence()
    assert ren.stats().frame_index == 3 and ren.stats().samples == 0 and c.retired_blocks == c.blocks > 0
    patch = patch_values(np.random.default_rng(17), v0, (5, 6, 7))
    ren.update_volume(patch, (30, 30, 30))
    ren.render()
    st, c = ren.stats(), ren.convergence()
    assert st.frame_index == 1 and st.samples > 0
    assert c.valid == 0 and c.retired_blocks == 0 and c.active_blocks == c.blocks > 0
    b = setup(ovr, made(), case, patched(v0, patch, (30, 30, 30)), accumulate=True)
    b.render()
    assert np.array_equal(bits(hip_frame(ovr, ren)[0]), bits(hip_frame(ovr, b)[0]))


def test_committed_setters_survive_and_the_data_range_fallback_follows(ovr, made):
    v0 = base_volume(ovr, np.float32, BIG)
    case = make_case(ovr, v0, tf="dense", vr=(1.0, -1.0))   # no valid transfer-function range, ever: the data range is in effect
    patch = patch_values(np.random.default_rng(18), v0, (9, 9, 9))
    patch[4, 4, 4] = 3.0
    lower = (28, 30, 31)

    def dress(ren):
        ren.set_clip_box((5.0, -np.inf, 8.0), (60.0, 55.0, np.inf))
        ren.set_light_direction((0.3, 0.8, 0.5), 1.25)
        ren.set_material(0.4, 0.5, 0.3, 12.0)
        ren.commit()

    a = setup(ovr, made(), case, v0)
    dress(a)
    a.render()
    clip, light = a.clip_box(), a.lighting()
    keep = (clip.enabled, tuple(clip.lower), tuple(clip.upper), tuple(clip.object_lower), tuple(clip.object_upper), tuple(light.direction), light.intensity, light.specular)
    assert a.volume_info().tf_upper == a.volume_info().data_upper < 3.0
    a.update_volume(patch, lower)
    clip, light = a.clip_box(), a.lighting()
    assert keep == (clip.enabled, tuple(clip.lower), tuple(clip.upper), tuple(clip.object_lower), tuple(clip.object_upper), tuple(light.direction), light.intensity, light.specular)
    assert a.volume_info().tf_upper == a.volume_info().data_upper == 3.0
    b = setup(ovr, made(), case, patched(v0, patch, lower))
    dress(b)
    assert info_tuple(a) == info_tuple(b)
    assert_same_frames(ovr, a, b, "dressed", layouts=(0, 3))


def test_the_tuner_starts_over(ovr, made):
    v0 = base_volume(ovr, np.float32, BIG)
    case = make_case(ovr, v0, tf="dense")
    ren = setup(ovr, made(), case, v0)   # automatic layout and pipeline, every sample shaded: the tuner probes
    seen = []
    for _ in range(3):
        ren.render()
        seen.append(ren.stats().tuning)
    assert seen[0] == 0 and seen[1] != 0, seen
    ren.update_volume(patch_values(np.random.default_rng(19), v0, (4, 4, 4)), (8, 8, 8))
    ren.render()
    assert ren.stats().tuning == 0   # the first frame of a configuration runs the rules' choice
    ren.render()
    assert ren.stats().tuning == 1   # ... and the candidates are timed again


# ---- 5. walk ------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_walk_of_updates_renders_and_edits(ovr, made):
    rng = np.random.default_rng(20)
    shadow = base_volume(ovr, np.float32, BIG).copy()
    case = make_case(ovr, shadow, tf="sparse")
    ren = setup(ovr, made(), case, shadow)
    tf, clip = "sparse", None
    for step in range(12):
        ext = [int(rng.integers(1, n + 1)) if rng.random() < 0.3 else int(rng.integers(1, 12)) for n in BIG]
        lower = [int(rng.integers(0, n - e + 1)) for n, e in zip(BIG, ext)]
        patch = patch_values(rng, shadow, ext[::-1], 0.0, 1.2)
        ren.update_volume(patch, lower)
        shadow = patched(shadow, patch, lower)
        if step % 3 == 0:
            ren.render()
        if step % 4 == 1:
            tf = "dense" if tf == "sparse" else "sparse"
            ren.set_transfer_function(*ovr.synth.make_tfn(tf, 256, np.float32))
            ren.commit()
        if step == 5:
            clip = ((10.0, 0.0, 0.0), (64.0, 67.0, 50.0))
            ren.set_clip_box(*clip)
            ren.commit()
        if step % 4 == 3:   # checkpoints after 4, 8 and 12 updates
            fresh = setup(ovr, made(), make_case(ovr, shadow, tf=tf), shadow)
            if clip:
                fresh.set_clip_box(*clip)
                fresh.commit()
            assert_same_layouts(ren, fresh, f"step {step}")
            assert info_tuple(ren) == info_tuple(fresh)
            assert_same_frames(ovr, ren, fresh, f"step {step}", layouts=(0, 2, 3), pipelines=(2,))
            fresh.close()


# ---- 6. device group ----------------------------------------------------------------------------------------------------------------------------------------

def test_a_device_group_updates_every_member(ovr, made):
    v0 = base_volume(ovr, np.float32, BIG)
    patch = patch_values(np.random.default_rng(21), v0, (13, 9, 20))
    lower = (24, 31, 17)
    case = make_case(ovr, v0, tf="dense")
    one, grp = setup(ovr, made(), case, v0), setup(ovr, made([0, 0, 0]), case, v0)
    for r in (one, grp):
        r.render()
        r.update_volume(patch, lower)
    first = observe(ovr, one)
    got = observe(ovr, grp)
    assert got[2] == first[2] and np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    want = layouts_of(one)
    for m in range(3):
        for k, (x, y) in enumerate(zip(layouts_of(grp, m), want)):
            assert np.array_equal(x, y), (m, k)
    with pytest.raises(RuntimeError, match="leaves the grid"):
        grp.update_volume(patch, (60, 31, 17))
    again = observe(ovr, grp)
    assert again[2] == first[2] and np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_volume_as_it_was(ovr, made):
    L = ovr._lib
    lib = L.load()
    v0 = base_volume(ovr, np.float32, BIG)
    case = make_case(ovr, v0)
    ren = setup(ovr, made(), case, v0)
    first = observe(ovr, ren)
    bytes0 = layouts_of(ren)
    data = np.full((2, 2, 2), 0.9, F)
    ptr = C.c_void_p(data.ctypes.data)
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    calls = {
        "null data": (None, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 1, 1), i3(2, 2, 2)),
        "null lower": (ptr, L.MEM_HOST, L.TYPE_FLOAT, None, i3(2, 2, 2)),
        "null extent": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 1, 1), None),
        "mem_kind": (ptr, 7, L.TYPE_FLOAT, i3(1, 1, 1), i3(2, 2, 2)),
        "another type": (ptr, L.MEM_HOST, L.TYPE_DOUBLE, i3(1, 1, 1), i3(2, 2, 2)),
        "an unknown type": (ptr, L.MEM_HOST, 12345, i3(1, 1, 1), i3(2, 2, 2)),
        "extent 0": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 1, 1), i3(2, 0, 2)),
        "extent < 0": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 1, 1), i3(2, 2, -1)),
        "lower < 0": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(-1, 1, 1), i3(2, 2, 2)),
        "past x": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(69, 1, 1), i3(2, 2, 2)),
        "past y": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 66, 1), i3(2, 2, 2)),
        "past z": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 1, 68), i3(2, 2, 2)),
        "overflow": (ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(1, 1, 1), i3(2, 2**31 - 1, 2)),
    }
    for what, args in calls.items():
        assert lib.ovr_hip_update_volume(ren._h, *args) == EINVAL, what
        again = observe(ovr, ren)
        assert again[2] == first[2] and np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), what
    for x, y in zip(layouts_of(ren), bytes0):
        assert np.array_equal(x, y)
    empty = made()
    assert lib.ovr_hip_update_volume(empty._h, ptr, L.MEM_HOST, L.TYPE_FLOAT, i3(0, 0, 0), i3(2, 2, 2)) == ESTATE
    n = C.c_uint64()
    assert lib.ovr_hip_get_volume_layout(empty._h, 0, 0, None, 0, C.byref(n)) == ESTATE
    assert lib.ovr_hip_get_volume_layout(ren._h, 0, 4, None, 0, C.byref(n)) == EINVAL
    assert lib.ovr_hip_get_volume_layout(ren._h, 1, 0, None, 0, C.byref(n)) == EINVAL


# ---- 8. host input and device input -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=lambda d: np.dtype(d).name)
def test_host_and_device_input_give_the_same_bytes(ovr, made, dtype):
    import torch
    v0 = base_volume(ovr, dtype, BIG)
    patch = patch_values(np.random.default_rng(22), v0, (13, 9, 20))
    lower = (24, 31, 17)
    case = make_case(ovr, v0)
    a, b = setup(ovr, made(), case, v0), setup(ovr, made(), case, v0)
    a.update_volume(patch, lower)
    b.update_volume(torch.from_numpy(patch).cuda(), lower)
    assert_same_layouts(a, b)
    ta, tb = a.update_times(), b.update_times()
    assert ta["copy_ms"] > 0 and tb["copy_ms"] == 0 and tb["alloc_ms"] == 0 and ta["total_ms"] >= ta["kernels_ms"] > 0 and tb["kernels_ms"] > 0
    a.update_volume(patch, lower)
    assert a.update_times()["alloc_ms"] == 0   # the staging buffer is kept
