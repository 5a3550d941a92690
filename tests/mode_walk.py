"""The walk of tests/test_mode_walk_model.py (no GPU) and tests/test_mode_walk_gpu.py: the frame kinds - march, projection, isosurfaces, translucent
isosurfaces - and the controls around them (camera kinds, clip box, shadow cache, light, material, ovr_hip_update_volume, skipping, layouts, pipeline,
convergence, sparse sampling and reconstruction, frame size, transfer function, new volumes, swaps, shards) changed in any order on ONE renderer.

A pure function: walk(seed, episodes, group) -> per episode the initial state and a list of transitions, each with its setter calls, the frames rendered behind
its commit, the COMPLETE committed state after it and its checked frames - the first one behind the commit and the last one -, each with the predicted
ovr_hip_stats.frame_index and the swaps / frames since the accumulation last started over.  Nothing here loads the HIP library: the generator, the frame-index model and reference A (the definition of a
frame: the CPU oracle for a plain march, projection.frame / isosurface.frame for the other kinds) run on a machine without a GPU.

What the walk leaves out, and why:
  - no swap while sparse sampling is on: a sparse frame writes only its sampled pixels, so after a swap the other set shows the pixels of the frames rendered
    into IT - the reference's two sets behave the same way (device_impl.cpp:226-239) - while the oracle models one set (tests/fuzz_states.py op 10);
  - no shard change under a gather: tiles.TileGather cuts its payload slots for one tile size (tests/fuzz_states.py op 9) - this walk runs no gather at all;
  - under an image shard of a single renderer the tiles of the other rank keep what they had (include/ovr_hip.h ovr_hip_set_image_shard; frame.cpp
    fill_target_params): they are no part of the frame, and both references compare the owned tiles only, as tests/fuzz_states.py does.
SUPPLIED shadow values, the plugin path and groups of distinct devices are not walked."""
import copy
import functools
import os
import sys

import numpy as np

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_R, os.path.join(_R, "tests"), os.path.join(_R, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import isosurface_cases as IC
import projection_cases as PC

F = np.float32
INF = float("inf")
SEED, EPISODES, GROUP_EPISODES, EXACT_EPISODES, TRANSITIONS = 222, 16, 4, 4, 8
FRAME_KINDS = ("march", "projection", "isosurface", "translucent")
VOLUMES = ("smooth", "ball", "slab", "plateau")
ISO_POOL = {"smooth": IC.NESTED["smooth"], "ball": IC.NESTED["ball"], "slab": (0.5, 0.8, 0.3, 0.65), "plateau": (101.0 / 255.0, 0.6, 0.3, 0.9)}
SIZES = ((40, 28), (37, 27), (45, 30), (33, 22), (41, 35))   # around PC.SIZE, ragged 8 x 8 blocks
# the boxes of tests/test_isosurface_gpu.py::test_clip_box and tests/test_projection_gpu.py::test_clip_box
CLIP_A, CLIP_B, CLIP_EMPTY = ((5.5, -INF, 3.0), (19.0, 20.25, INF)), ((5.5, -INF, 3.0), (27.0, 20.25, INF)), ((10.0, 0.0, 0.0), (10.0, 33.0, 18.0))
LIGHTS = ((0.3, 0.8, -0.52), (-0.5, 0.6, 0.62), (0.7, 0.2, 0.68))
REFERENCE_MATERIAL = (0.5, 0.5, 0.0, 0.0)
MATERIALS = ((0.3, 0.6, 0.4, 12.0), (0.6, 0.9, 0.4, 40.0))
MARCHED, CACHED = 0, 1
OFF, ESTIMATE, ADAPTIVE = 0, 1, 2
UNVERIFIED_THRESHOLD = 1.0e-3   # ADAPTIVE where no whole-frame definition exists to derive a threshold from
_noise = None


def noise_tile():
    global _noise
    if _noise is None:
        _noise = np.random.default_rng(5).random((16, 16, 64), dtype=F)
        _noise.setflags(write=False)
    return _noise


# ---- the frame index ------------------------------------------------------------------------------------------------------------------------------
# The sources as tests/commit_walk.py's literals know them: a call of a queued setter starts the accumulation over whatever its value (the projection and
# isosurface setters are recorded with the shading mode: "EVERY call resets the accumulation", include/ovr_hip.h); light, material, clip box and shadow cache
# only with another value; LDS staging, layout choice, pipeline, skipping and a swap never.  Without accumulation no frame consumes the reset: the index runs on.
ALWAYS = frozenset(("fbsize", "camera", "tf", "focus", "spp", "sparse", "accumulation", "rate", "shading", "projection", "isosurfaces", "jitter", "convergence",
                    "reconstruction", "shard", "upload", "update", "noise"))
ON_DIFFERS = frozenset(("light", "material", "clip", "shadow"))
NEVER = frozenset(("lds", "layout", "pipeline", "skipping", "swap"))


def starts_over(source, differs):
    if source in ALWAYS:
        return True
    if source in ON_DIFFERS:
        return bool(differs)
    assert source in NEVER, source
    return False


class IndexModel:
    """ovr_hip_stats.frame_index and what happened since the accumulation last started over: 's' a swap, 'r' a frame"""

    def __init__(self, accumulate=True):
        self.pending, self.index, self.accumulate, self.history = True, 0, accumulate, []

    def call(self, source, differs=True):
        if starts_over(source, differs):
            self.pending = True

    def swap(self):
        self.history.append("s")

    def render(self):
        if self.accumulate and self.pending:
            self.pending, self.index, self.history = False, 0, []
        self.index += 1
        self.history.append("r")
        return self.index


# ---- the state ------------------------------------------------------------------------------------------------------------------------------------
def frame_kind(s):
    if s["iso"]:
        return "translucent" if s["opacities"] is not None and min(s["opacities"]) < 1.0 else "isosurface"
    return "projection" if s["projection"] else "march"


def dtype_of(s):
    return np.dtype(s["dtype"])


def full_scale(dtype):
    return 65535.0 if np.dtype(dtype) == np.uint16 else 255.0 if np.dtype(dtype) == np.uint8 else 1.0


def patch_array(s, patch):
    """a patch (lower xyz, shape zyx, fraction of full scale) as the array ovr_hip_update_volume takes"""
    _, shape, frac = patch
    dt = dtype_of(s)
    return np.full(shape, frac, F) if dt == np.float32 else np.full(shape, int(round(frac * full_scale(dt))), dt)


def volume_of(s):
    """the resident volume: the case's array with the state's patches applied on the host"""
    v = IC.volume(s["volume"], dtype_of(s), s["dims"])
    if s["patches"]:
        v = v.copy()
        for p in s["patches"]:
            (x, y, z), (pz, py, px), _ = p
            v[z:z + pz, y:y + py, x:x + px] = patch_array(s, p)
    return v


def centre(dims):
    return tuple(d / 2.0 for d in dims)


def named_camera(name, dims):
    """PC.CAMERAS and IC.BEHIND as they are for the 40 x 33 x 18 volume; for the smaller one moved to its centre and half as far away"""
    eye, at, up = IC.BEHIND if name == "behind" else PC.CAMERAS[name]
    c, k = np.array(centre(dims)), (1.0 if tuple(dims) == tuple(PC.DIMS[0]) else 0.5)
    return tuple(float(x) for x in c + (np.array(eye) - np.array(at)) * k), tuple(float(x) for x in c), up


def tfn_of(ovr, s):
    kind, n = s["tf"]
    colors, alphas, vr = ovr.synth.make_tfn(kind, n, dtype_of(s))
    return colors, alphas, (s["vr"] if s["vr"] is not None else (float(vr[0]), float(vr[1])))


def case_of(ovr, s):
    """the dict tests/helpers.py's oracle_scene and the feature tests' _check_frame read"""
    colors, alphas, vr = tfn_of(ovr, s)
    return dict(vol=volume_of(s), colors=colors, alphas=alphas, vr=vr, cam=(s["eye"], s["at"], s["up"]), size=s["size"], shading=s["shading"], rate=s["rate"], spp=s["spp"],
                convention=0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), fovy=s["fovy"])


def owned_mask(ovr, s):
    """(H, W) bool of the pixels a single renderer under an image shard draws; None: all of them"""
    if not s["shard"] or s["shard"][1] <= 1:
        return None
    rank, world, tw, th = s["shard"]
    w, h = s["size"]
    mask = np.zeros((h, w), bool)
    for tx, ty in ovr.tiles.owned_tiles(w, h, tw, th, rank, world):
        mask[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = True
    return mask


# ---- reference A: the definition ------------------------------------------------------------------------------------------------------------------
def plain_march(s):
    """the states whose frame the CPU oracle defines: perspective camera, no clip box, and - where the shading mode reads them at all - the reference's light
    and material (GRADIENT, FULL) and marched shadows (FULL)"""
    lit = s["shading"] == 0 or (s["light"] == (None, 1.0) and s["material"] == REFERENCE_MATERIAL)
    return (frame_kind(s) == "march" and s["ortho"] is None and s["clip"] is None and lit and (s["shading"] < 2 or s["shadow"][0] == MARCHED)
            and s["convergence"][0] != ADAPTIVE and not (s["sparse"] and s["reconstruction"]))


def has_definition(s, frame_index):
    """whether reference A exists for the checked frame of a state: the oracle accumulates; the numpy models render ONE frame of all pixels - the frame of
    index 1, any frame without accumulation, and the second accumulated frame where every frame is the same frame (one sample per pixel, no jitter):
    (a + a) / 2 == a bit for bit, as tests/test_projection_gpu.py::test_accumulation_spp_and_jitter holds it"""
    if plain_march(s):
        return True
    if frame_kind(s) == "march" or s["convergence"][0] == ADAPTIVE or s["sparse"] or owned_mask_needed(s):
        return False
    if s["spp"] > 1 and not s["jitter"]:
        return False   # (the models do not restate the RandomTEA jitter)
    return frame_index == 1 or not s["accumulate"] or (frame_index == 2 and s["spp"] == 1 and not s["jitter"])


def model_frame_index(s, frame_index):
    """the index of the ONE frame the model renders for a checked frame (has_definition)"""
    return 1 if s["accumulate"] else int(frame_index)


def owned_mask_needed(s):
    return bool(s["shard"]) and s["shard"][1] > 1


def march_definition(ovr, O, s, frame_index):
    """(rgba, counters) of the oracle's frame, as tests/fuzz_states.py::check asks for it"""
    from helpers import oracle_scene
    kw = {}
    if s["sparse"]:
        kw.update(sparse=True, focus=s["focus"], noise=noise_tile())
    if owned_mask_needed(s):
        kw.update(shard=s["shard"])
    if s["jitter"]:
        kw.update(jitter=1, noise=noise_tile())
    ref, _, cnt = oracle_scene(O, case_of(ovr, s), **kw).render(frames=int(frame_index), accumulate=s["accumulate"])
    return ref, cnt


def model_definition(ovr, s, frame_index, exact=False):
    """(rgba, layer, counters) of projection.frame / isosurface.frame for the state's clip box, skipping, spp, noise tile, frame index, camera kind, light,
    material and opacities; exact: the exact-parity library runs (no product_sampler for the 8-bit volumes)"""
    P, I, K = ovr.projection, ovr.isosurface, ovr.camera
    vol = volume_of(s)
    w, h = s["size"]
    basis = K.basis(s["eye"], s["at"], s["up"], w, h, s["fovy"], s["ortho"])
    colors, alphas, vr = tfn_of(ovr, s)
    ct, at = PC.tables(colors, alphas)
    clip = None
    if s["clip"] is not None:
        inv, wp = ovr.clipping.volume_constants(s["dims"])
        clip = ovr.clipping.object_box(s["clip"][0], s["clip"][1], inv, wp)
    kw = dict(clip=clip, skipping=s["skipping"], spp=s["spp"], noise=noise_tile() if s["jitter"] else None, frame_index=int(frame_index),
              camera_kind=K.ORTHOGRAPHIC if s["ortho"] is not None else K.PERSPECTIVE)
    tf_range = P.normalized_range(vr, vol.dtype)
    if frame_kind(s) == "projection":
        return P.frame(vol, basis, (w, h), s["rate"], s["projection"], ct, at, tf_range, **kw)
    iso = np.sort(np.asarray(s["iso"], F))
    op = None if s["opacities"] is None else I.opacities_of(s["opacities"], s["iso"])
    return I.frame(vol, basis, (w, h), s["rate"], iso, ct, tf_range, shading=s["shading"], light=s["light"][0], intensity=s["light"][1], material=s["material"],
                   sampler=None if exact else I.product_sampler(vol), opacities=op, **kw)


# ---- the generator --------------------------------------------------------------------------------------------------------------------------------
# Every kind of transition twice and more, the changes of the frame kind most often: dealt from one shuffled deck over all episodes, so that a walk of
# 16 x 8 transitions holds every entry of the deck whatever the seed.  `kind` picks, per visit, the ordered pair of frame kinds seen least so far; `clip`
# what has happened least to a box in the state it is in.  What still depends on the seed (which state an update or ADAPTIVE meets, how many frames have a
# definition) is what tests/test_mode_walk_model.py holds the committed SEED to.
DECK = (["kind"] * 34 + ["camera_orthographic_auto"] * 2 + ["camera_orthographic"] * 2 + ["camera_perspective"] * 2 + ["camera_move"] * 2 + ["camera_axis"] * 2 + ["camera_fov"] * 2 + ["clip"] * 11 +
        ["shadow_mode"] * 4 + ["shadow_cell"] * 2 + ["shadow_same"] * 2 + ["light_direction"] * 2 + ["light_longer"] * 2 +
        ["light_same"] * 2 + ["material_new"] * 2 + ["material_back"] * 2 + ["update_cross"] * 4 + ["update_raises_maximum"] * 2 + ["update_removes_maximum"] * 2 + ["skipping"] * 4 + ["layout"] * 2 +
        ["pipeline"] * 2 + ["lds"] * 2 + ["shading"] * 2 + ["rate"] * 2 + ["spp"] * 2 + ["jitter"] * 2 + ["accumulation"] * 2 + ["convergence_off"] * 2 + ["convergence_estimate"] * 2 + ["convergence_adaptive"] * 3 + ["sparse"] * 2 +
        ["reconstruction_fill"] * 2 + ["reconstruction_off"] * 2 + ["fbsize"] * 2 + ["tf"] * 2 + ["value_range"] * 2 + ["new_volume"] * 2 + ["swap"] * 2 + ["shard"] * 2)
assert len(DECK) == EPISODES * TRANSITIONS


def _f32(t):
    return None if t is None else tuple(float(F(x)) for x in t)


def _iso_values(rng, s, n=None):
    n = int(rng.integers(1, 5)) if n is None else n
    pool = np.array(ISO_POOL[s["volume"]])
    pick = np.sort(pool)[:n][rng.permutation(n)]    # the n lowest - the widest level sets - as given: unsorted, the setter sorts them
    return tuple(float(F(x * (65535.0 if dtype_of(s) == np.uint16 else 1.0))) for x in pick)


def _opacities(rng, n, ones=False):
    if ones:
        return (1.0,) * n
    a = [float(rng.choice([0.25, 0.3, 0.4, 0.5, 0.6, 1.0])) for _ in range(n)]
    if min(a) == 1.0:
        a[int(rng.integers(n))] = 0.4
    return tuple(a)


def _initial(rng):
    dims = PC.DIMS[int(rng.integers(2))]
    name = str(rng.choice(["oblique", "axis", "behind"]))
    eye, at, up = named_camera(name, dims)
    return dict(volume=str(rng.choice(VOLUMES)), dtype=np.dtype(PC.DTYPES[int(rng.integers(3))]).name, dims=dims, patches=[], eye=eye, at=at, up=up, fovy=PC.FOVY, ortho=None,
                size=SIZES[0], tf=("sparse", 16), vr=None, rate=float(rng.choice(PC.RATES)), shading=int(rng.integers(3)), spp=1, jitter=0, accumulate=True, sparse=False,
                focus=((0.5, 0.45), 0.35, 0.15), light=(None, 1.0), material=REFERENCE_MATERIAL, clip=(None, None, None, CLIP_A, CLIP_B)[int(rng.integers(5))],
                shadow=(CACHED if rng.integers(4) == 0 else MARCHED, 4), projection=0, iso=(), opacities=None, skipping=bool(rng.integers(2)), layout=-1, pipeline=0, lds=False, convergence=(OFF, 0.0), reconstruction=0, shard=None)


def _camera_call(s):
    return ("set_camera", s["eye"], s["at"], s["up"], s["fovy"], s["ortho"])


def _iso_call(s):
    return ("set_isosurfaces", s["iso"], s["opacities"])


def _to_kind(rng, s, target, calls, src, labels, pairs):
    """the setter calls that take the frame kind to `target`; a committed projection mode stays committed under isovalues and resumes at n = 0"""
    cur = frame_kind(s)
    if target in ("isosurface", "translucent"):
        n = 1 + pairs.get("isovalues", 0) % 4     # 1 ... 4 isovalues in turn
        pairs["isovalues"] = pairs.get("isovalues", 0) + 1
        s["iso"] = _iso_values(rng, s, n)
        if target == "translucent":
            s["opacities"], label = _opacities(rng, n), "layers"
        elif pairs.get("opaque", 0) % 3 == 1:
            s["opacities"], label = _opacities(rng, n, ones=True), "layers_ones"
        else:
            s["opacities"], label = None, "isosurfaces"
        if target == "isosurface":
            pairs["opaque"] = pairs.get("opaque", 0) + 1
        if cur == "projection":
            label += "_over_projection"
        calls.append(_iso_call(s)); src.append(("isosurfaces", True)); labels.append(label)
        return
    if s["iso"]:
        s["iso"], s["opacities"] = (), None
        calls.append(("set_isosurfaces", (), None)); src.append(("isosurfaces", True))
        labels.append("projection_resumes" if s["projection"] and target == "projection" else "isosurfaces_off")
    if target == "projection" and (not s["projection"] or cur == "projection"):
        pairs["modes"] = pairs.get("modes", 0) + (2 if 1 + pairs.get("modes", 0) % 3 == s["projection"] else 1)
        s["projection"] = 1 + (pairs["modes"] - 1) % 3   # the modes in turn
        calls.append(("set_projection", s["projection"])); src.append(("projection", True)); labels.append("projection")
    if target == "march" and s["projection"]:
        s["projection"] = 0
        calls.append(("set_projection", 0)); src.append(("projection", True)); labels.append("projection_off")


def _adaptive_threshold(ovr, O, s):
    """a threshold at which some but not all blocks retire after frame 2: the median of the positive block errors of the definition's first two frames
    (blue-noise jitter on: the frames differ).  Returns (threshold, verified)"""
    M = ovr.convergence
    if s["sparse"] or owned_mask_needed(s):
        return UNVERIFIED_THRESHOLD, False
    probe = dict(s, convergence=(OFF, 0.0), accumulate=False)
    if plain_march(probe):
        frames = [march_definition(ovr, O, dict(probe, accumulate=False), k)[0] for k in (1, 2)]
    elif frame_kind(s) != "march":
        frames = [model_definition(ovr, probe, k)[0] for k in (1, 2)]
    else:
        return UNVERIFIED_THRESHOLD, False
    frames = [np.nan_to_num(f) for f in frames]
    sums = M.accumulate(frames)
    E = M.block_errors(sums[1][1], sums[1][2], 2)
    pos = np.unique(E[E > 0])
    if len(pos) < 2:
        return UNVERIFIED_THRESHOLD, False
    return float(pos[(len(pos) - 1) // 2]), True


def _transition(ovr, O, rng, s, op, group, pairs):
    """applies one operation to the state s in place; returns (labels, calls, sources, frames or None, extra)"""
    calls, src, labels, frames, extra = [], [], [op], None, {}
    dims = s["dims"]
    if op == "kind":
        cur = frame_kind(s)
        order = [FRAME_KINDS[i] for i in rng.permutation(4)]
        target = min(order, key=lambda k: pairs.get((cur, k), 0) + (0.5 if k == cur else 0))
        if cur == "projection" and pairs.get("resumes", 0) >= 2 and pairs.get("offs", 0) < 3:   # set_projection(0): the march again
            target, pairs["offs"] = "march", pairs.get("offs", 0) + 1
        elif pairs.get("resumes", 0) < 2 and s["projection"]:   # projection -> isovalues over it -> the projection resumes at n = 0 (include/ovr_hip.h)
            target = "projection" if s["iso"] else str(rng.choice(["isosurface", "translucent"]))
            pairs["resumes"] = pairs.get("resumes", 0) + (1 if s["iso"] else 0)
        labels.pop()
        _to_kind(rng, s, target, calls, src, labels, pairs)
        if not calls:   # (the march stays the march: a commit with nothing queued, then frames)
            labels.append("commit_only")
    elif op in ("camera_orthographic_auto", "camera_orthographic", "camera_perspective"):   # (the same kind again is a camera call like any other)
        if op == "camera_orthographic_auto":
            s["ortho"] = float(ovr.camera.auto_height(s["eye"], s["at"], s["fovy"]))
        else:
            s["ortho"] = None if op == "camera_perspective" else float(rng.choice([30.0, 38.0])) * max(s["dims"]) / 40.0
        calls.append(_camera_call(s)); src.append(("camera", True))
    elif op == "camera_move":
        s["eye"], s["at"], s["up"] = named_camera(str(rng.choice(["oblique", "axis", "behind"])), dims)
        calls.append(_camera_call(s)); src.append(("camera", True))
    elif op == "camera_axis":
        k, sign = int(rng.integers(3)), float(rng.choice([-1.0, 1.0]))
        if s["volume"] == "slab":
            k = 2   # (along x or y the slab's level sets are seen edge-on: a line of pixels)
        c = np.array(centre(dims))
        s["eye"] = tuple(float(x) for x in c + np.eye(3)[k] * sign * 2.4 * max(dims))
        s["at"], s["up"] = tuple(float(x) for x in c), ((0.0, 1.0, 0.0) if k != 1 else (0.0, 0.0, 1.0))
        calls.append(_camera_call(s)); src.append(("camera", True))
    elif op == "camera_fov":
        if s["ortho"] is None:
            s["fovy"] = float(rng.choice([f for f in (28.0, 40.0, 55.0) if f != s["fovy"]]))
        else:
            s["ortho"] = float(rng.choice([h for h in (30.0, 38.0, 46.0) if h * max(dims) / 40.0 != s["ortho"]])) * max(dims) / 40.0
        calls.append(_camera_call(s)); src.append(("camera", True))
    elif op == "clip":
        # what can happen to the box there is: without one, one is set; with one, the same again, the other one (wider or narrower), none, or the empty one -
        # whichever the walk has done least so far.  (A box that only ever appears would leave the schedule's block test of a WIDER box untried.)
        before = s["clip"]
        options = ["clip_set", "clip_empty"] if before is None else ["clip_remove", "clip_other", "clip_set"] if before == CLIP_EMPTY else ["clip_same", "clip_other", "clip_remove", "clip_empty"]
        op = min([options[i] for i in rng.permutation(len(options))], key=lambda o: pairs.get(o, 0))
        pairs[op] = pairs.get(op, 0) + 1
        labels[0] = op
        if op == "clip_set":
            s["clip"] = CLIP_A
        elif op == "clip_other":
            s["clip"] = CLIP_B if before != CLIP_B else CLIP_A
        elif op == "clip_remove":
            s["clip"] = None
        elif op == "clip_empty":
            s["clip"] = CLIP_EMPTY
        calls.append(("set_clip_box",) + (s["clip"] if s["clip"] is not None else (None, None))); src.append(("clip", s["clip"] != before))
    elif op.startswith("shadow_"):
        before = s["shadow"]
        if op == "shadow_mode":
            s["shadow"] = (CACHED if before[0] == MARCHED else MARCHED, before[1])
        elif op == "shadow_cell":
            s["shadow"] = (before[0], int(rng.choice([c for c in (2, 3, 4) if c != before[1]])))
        calls.append(("set_shadow_cache",) + s["shadow"]); src.append(("shadow", s["shadow"] != before))
    elif op.startswith("light_"):
        before = s["light"]
        if op == "light_direction":
            choices = [l for l in LIGHTS + (None,) if l != before[0]]
            s["light"] = (choices[int(rng.integers(len(choices)))], float(rng.choice([1.0, 1.0, 1.5])))
        elif op == "light_longer":   # a longer vector in the same direction: another value, the same unit vector (commit_plan.hpp kLightVector / kLightDirection)
            v = before[0] if before[0] is not None else tuple(float(x) for x in ovr.lighting.LITERAL_LIGHT)
            s["light"] = (tuple(2.0 * x for x in v), before[1])
        calls.append(("set_light_direction",) + s["light"]); src.append(("light", (_f32(s["light"][0]), s["light"][1]) != (_f32(before[0]), before[1])))
    elif op.startswith("material_"):
        before = s["material"]
        s["material"] = REFERENCE_MATERIAL if op == "material_back" else [m for m in MATERIALS if m != before][int(rng.integers(len([m for m in MATERIALS if m != before])))]
        calls.append(("set_material",) + s["material"]); src.append(("material", s["material"] != before))
    elif op in ("update_cross", "update_raises_maximum", "update_removes_maximum"):
        nx, ny, nz = dims
        vol = volume_of(s).astype(np.float64) / full_scale(dtype_of(s))
        if op == "update_cross":   # the box of tests/test_isosurface_gpu.py (dim cells behind the slab), moved into the smaller volume: its cells' ranges cross the isovalues
            lower, shape = ((14, 12, 15), (3, 9, 11)) if nz >= 18 else ((8, 6, 13), (3, 9, 11))
            region = vol[lower[2]:lower[2] + 3, lower[1]:lower[1] + 9, lower[0]:lower[0] + 11]
            frac = 0.97 if region.mean() < 0.5 else 0.02
        elif op == "update_raises_maximum":   # raises the maximum: full scale in a box across a macrocell border
            lower, shape, frac = ((13, 12, 8) if nz >= 18 else (8, 6, 8)), (6, 9, 11), 1.0
        else:                        # removes the maximum: a dim box over the brightest voxel
            z, y, x = (int(i) for i in np.unravel_index(int(np.argmax(vol)), vol.shape))
            lower = (max(min(x - 3, nx - 7), 0), max(min(y - 3, ny - 7), 0), max(min(z - 2, nz - 5), 0))
            shape, frac = (5, 7, 7), 0.05
        s["patches"] = s["patches"] + [(lower, shape, frac)]
        calls.append(("update_volume", lower, shape, frac)); src.append(("update", True))
        extra["update_under"] = dict(iso_and_skipping=bool(s["iso"]) and s["skipping"], cached=s["shadow"][0] == CACHED)
    elif op == "skipping":
        s["skipping"] = not s["skipping"]
        calls.append(("set_empty_space_skipping", s["skipping"])); src.append(("skipping", True))
    elif op == "layout":
        s["layout"] = int(rng.choice([l for l in (-1, 0, 1, 2, 3) if l != s["layout"]]))
        calls.append(("set_layout_choice", s["layout"])); src.append(("layout", True))
    elif op == "pipeline":
        s["pipeline"] = int(rng.choice([p for p in (0, 1, 2) if p != s["pipeline"]]))
        calls.append(("set_shading_pipeline", s["pipeline"])); src.append(("pipeline", True))
    elif op == "lds":
        s["lds"] = not s["lds"]
        calls.append(("set_lds_staging", s["lds"])); src.append(("lds", True))
    elif op == "shading":
        s["shading"] = int(rng.choice([m for m in (0, 1, 2) if m != s["shading"]]))
        calls.append(("set_shading", s["shading"])); src.append(("shading", True))
    elif op == "rate":
        s["rate"] = float([r for r in PC.RATES if r != s["rate"]][0])
        calls.append(("set_volume_sampling_rate", s["rate"])); src.append(("rate", True))
    elif op == "spp":
        s["spp"] = int(rng.choice([n for n in (1, 2, 3) if n != s["spp"]]))
        calls.append(("set_sample_per_pixel", s["spp"])); src.append(("spp", True))
    elif op == "jitter":
        s["jitter"] = 1 - s["jitter"]
        calls.append(("set_pixel_jitter", s["jitter"])); src.append(("jitter", True))
    elif op == "accumulation":
        s["accumulate"] = not s["accumulate"]
        calls.append(("set_frame_accumulation", s["accumulate"])); src.append(("accumulation", True))
    elif op.startswith("convergence_"):
        mode = {"convergence_off": OFF, "convergence_estimate": ESTIMATE, "convergence_adaptive": ADAPTIVE}[op]
        if mode == ADAPTIVE:   # with accumulation and the blue-noise jitter: the frames differ, so the blocks' errors do; three frames: past the even frame that retires
            if not s["accumulate"]:
                s["accumulate"] = True
                calls.append(("set_frame_accumulation", True)); src.append(("accumulation", True))
            if not s["jitter"]:
                s["jitter"] = 1
                calls.append(("set_pixel_jitter", 1)); src.append(("jitter", True))
            t, verified = _adaptive_threshold(ovr, O, s)
            s["convergence"], frames = (ADAPTIVE, t), 3
            extra["adaptive_verified"] = verified
        else:
            s["convergence"] = (mode, 0.0)
        calls.append(("set_convergence",) + s["convergence"]); src.append(("convergence", True))
    elif op == "sparse":
        s["sparse"] = not s["sparse"]
        if s["sparse"]:
            s["focus"] = ((float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.7))), float(rng.uniform(0.2, 0.5)), float(rng.uniform(0.05, 0.3)))
            calls.append(("set_focus",) + s["focus"]); src.append(("focus", True))
        calls.append(("set_sparse_sampling", s["sparse"])); src.append(("sparse", True))
    elif op in ("reconstruction_fill", "reconstruction_off"):
        # (include/ovr_hip.h ovr_hip_set_reconstruction: a device group refuses every mode but OFF - there FILL is replaced by OFF)
        s["reconstruction"] = 1 if op == "reconstruction_fill" and not group else 0
        calls.append(("set_reconstruction", s["reconstruction"])); src.append(("reconstruction", True))
    elif op == "fbsize":
        s["size"] = SIZES[int(rng.choice([i for i in range(len(SIZES)) if SIZES[i] != s["size"]]))]
        calls.append(("set_fbsize", s["size"])); src.append(("fbsize", True))
    elif op == "tf":
        s["tf"], s["vr"] = (str(rng.choice(["sparse", "dense", "bumps"])), int(rng.choice([16, 64, 256]))), None
        calls.append(("set_transfer_function",)); src.append(("tf", True))
    elif op == "value_range":
        lo0, hi0 = ovr.synth.make_tfn("dense", 8, dtype_of(s))[2]
        a, b = sorted(rng.uniform(0.0, 1.0, 2))
        s["vr"] = (float(F(lo0 + a * (hi0 - lo0))), float(F(lo0 + max(b, a + 0.05) * (hi0 - lo0))))
        calls.append(("set_transfer_function",)); src.append(("tf", True))
    elif op == "new_volume":   # another dtype and other dims; committed isovalues are in the old volume's units: they are set again for the new one
        s["dims"] = [d for d in PC.DIMS if d != dims][0]
        s["dtype"] = np.dtype([d for d in PC.DTYPES if np.dtype(d).name != s["dtype"]][int(rng.integers(2))]).name
        s["volume"], s["patches"], s["vr"] = str(rng.choice(VOLUMES)), [], None
        s["eye"], s["at"], s["up"] = named_camera("oblique", s["dims"])
        calls.append(("new_volume",)); src.extend([("tf", True), ("camera", True), ("upload", True), ("sparse", True)])
        if s["iso"]:
            s["iso"] = _iso_values(rng, s, len(s["iso"]))
            calls.append(_iso_call(s)); src.append(("isosurfaces", True))
    elif op == "swap":
        if s["sparse"]:
            labels[0] = "render_only"
        else:
            calls.append(("swap",)); src.append(("swap", True))
    elif op == "shard":
        if group:   # a group deals its tiles itself: the transition is a tile-size change, every frame stays the whole frame
            s["shard"] = (0, 1, int(rng.choice([4, 8, 16, 24])), int(rng.choice([4, 8, 16])))
        else:
            s["shard"] = (0, 1, 16, 16) if owned_mask_needed(s) else (int(rng.integers(2)), 2, int(rng.choice([8, 16])), int(rng.choice([8, 16])))
        calls.append(("set_image_shard",) + s["shard"]); src.append(("shard", True))
    else:
        raise ValueError(op)
    return labels, calls, src, frames, extra


@functools.lru_cache(maxsize=None)
def walk(seed=SEED, episodes=EPISODES, group=False):
    """[dict(initial=state, transitions=[dict(labels, calls, frames, state, kind, checks=[dict(after, frame_index, history, definition)], ...)])] - deterministic"""
    import ovr_amd as ovr   # (the numpy models and the synthetic inputs; the HIP library is loaded by _lib.load() alone, which nothing here calls)
    import oracle as O
    deck = list(DECK)
    order = np.random.default_rng([seed, 0]).permutation(len(deck))
    deck = [deck[i] for i in order]
    pairs, out = {}, []
    for ep in range(episodes):
        rng = np.random.default_rng([seed, 1, ep])
        s = _initial(rng)
        idx = IndexModel(True)
        idx.render()
        first = dict(labels=["initial"], calls=[], frames=1, state=copy.deepcopy(s), kind=frame_kind(s), checks=[dict(after=1, frame_index=1, history=list(idx.history), definition=has_definition(s, 1))])
        ts, last = [], frame_kind(s)
        for k in range(TRANSITIONS):
            op = deck[(ep * TRANSITIONS + k) % len(deck)]
            labels, calls, src, frames, extra = _transition(ovr, O, rng, s, op, group, pairs)
            for source, differs in src:
                if source == "swap":
                    idx.swap()
                idx.call(source, differs)
            idx.accumulate = s["accumulate"]
            frames = int(rng.choice([1, 1, 2, 3])) if frames is None else frames
            checks = []   # the first frame behind the commit and the last one
            for n in range(1, frames + 1):
                fi = idx.render()
                if n in (1, frames):
                    checks.append(dict(after=n, frame_index=fi, history=list(idx.history), definition=has_definition(s, fi)))
            kind = frame_kind(s)
            pairs[(last, kind)] = pairs.get((last, kind), 0) + 1
            last = kind
            ts.append(dict(labels=labels, calls=calls, frames=frames, state=copy.deepcopy(s), kind=kind, checks=checks, **extra))
        out.append(dict(episode=ep, seed=seed, group=group, initial=first, transitions=ts))
    return out


def episode(seed, ep, group=False, episodes=EPISODES):
    return walk(seed, episodes, group)[ep]


def describe(t):
    s = t["state"]
    return (f"{'+'.join(t['labels'])}: {t['calls']} -> {t['frames']} frame(s), frame_index {[c['frame_index'] for c in t['checks']]}, {t['kind']}"
            f" [{s['volume']} {s['dtype']} {s['dims']} size {s['size']} ortho {s['ortho']} clip {s['clip']} shadow {s['shadow']} projection {s['projection']} iso {s['iso']} / {s['opacities']}"
            f" skipping {s['skipping']} sparse {s['sparse']} recon {s['reconstruction']} conv {s['convergence']} acc {s['accumulate']} spp {s['spp']} jitter {s['jitter']} shard {s['shard']}]")
