"""The walk of tests/mode_walk.py checked on the CPU, for the seed and the episode counts tests/test_mode_walk_gpu.py runs: that it is deterministic, that it
holds every kind of transition, every frame kind and every ordered pair of them, that its states draw something, and that its frame-index model agrees
with the literals of tests/commit_walk.py.  A walk that tests little must not pass unnoticed.  No GPU: the HIP library is never loaded here."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import commit_walk
import mode_walk as W

# every kind of transition the walk is to hold (at least twice each)
TRANSITION_KINDS = (
    "projection", "projection_off", "isosurfaces", "layers", "layers_ones", "isosurfaces_off", "projection_resumes",
    "camera_orthographic_auto", "camera_orthographic", "camera_perspective", "camera_move", "camera_axis", "camera_fov",
    "clip_set", "clip_same", "clip_other", "clip_remove", "clip_empty", "shadow_mode", "shadow_cell", "shadow_same", "light_direction", "light_longer", "light_same",
    "material_new", "material_back", "update_cross", "update_raises_maximum", "update_removes_maximum", "skipping", "layout", "pipeline", "lds", "shading", "rate", "spp",
    "jitter", "accumulation", "convergence_off", "convergence_estimate", "convergence_adaptive", "sparse", "reconstruction_fill", "reconstruction_off", "fbsize", "tf",
    "value_range", "new_volume", "swap", "shard")


@pytest.fixture(scope="module")
def walk():
    return W.walk(W.SEED, W.EPISODES, False)


def _checked(walk):
    """(transition, check) of every checked frame, in order"""
    for e in walk:
        for t in [e["initial"]] + e["transitions"]:
            for c in t["checks"]:
                yield e, t, c


def test_the_generator_is_deterministic_and_loads_no_hip_library(walk):
    W.walk.cache_clear()
    again = W.walk(W.SEED, W.EPISODES, False)
    assert repr(again) == repr(walk) and again is not walk
    assert W.episode(W.SEED, 3)["transitions"] == again[3]["transitions"]
    group = W.walk(W.SEED, W.GROUP_EPISODES, True)
    W.walk.cache_clear()
    assert repr(W.walk(W.SEED, W.GROUP_EPISODES, True)) == repr(group)
    probe = "import sys; sys.path.insert(0, %r); import mode_walk as W; W.walk(W.SEED, 2, False); import ovr_amd; assert ovr_amd._lib._lib is None" % os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", probe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, "the walk loaded the HIP library: " + out.stderr[-1500:]
    assert len(walk) == W.EPISODES and all(len(e["transitions"]) == W.TRANSITIONS for e in walk)
    for e in group:   # a group renders whole frames and refuses reconstruction
        for t in e["transitions"]:
            assert t["state"]["reconstruction"] == 0 and (not t["state"]["shard"] or t["state"]["shard"][1] == 1)


def test_every_transition_kind_frame_kind_and_pair_occurs(walk):
    labels = collections.Counter()
    for e in walk:
        for t in e["transitions"]:
            labels.update(l.replace("_over_projection", "") for l in t["labels"])
            assert 1 <= t["frames"] <= 3 and t["checks"][0]["after"] == 1 and t["checks"][-1]["after"] == t["frames"]
    missing = [k for k in TRANSITION_KINDS if labels[k] < 2]
    assert not missing, (missing, labels)
    over = sum(1 for e in walk for t in e["transitions"] for l in t["labels"] if l.endswith("_over_projection"))
    assert over >= 2, "isovalues committed over a committed projection mode"
    kinds, pairs, last = collections.Counter(), collections.Counter(), None
    with_a = 0
    for e, t, c in _checked(walk):
        kinds[t["kind"]] += 1
        with_a += bool(c["definition"])
        if last is not None and last != t["kind"]:
            pairs[(last, t["kind"])] += 1
        last = t["kind"]
    assert all(kinds[k] >= 6 for k in W.FRAME_KINDS), kinds
    assert len(pairs) == 12, sorted(pairs)
    assert 2 * with_a >= sum(kinds.values()), (with_a, sum(kinds.values()))
    print(f"checked frames per kind {dict(kinds)}, with reference A {with_a} of {sum(kinds.values())}")
    # the values the setters are walked through
    modes = {t["state"]["projection"] for e in walk for t in e["transitions"]}
    n_iso = {len(t["state"]["iso"]) for e in walk for t in e["transitions"]}
    assert modes == {0, 1, 2, 3} and n_iso >= {0, 1, 2, 3, 4}, (modes, n_iso)


def test_updates_and_adaptive_episodes_meet_the_state_they_are_for(walk):
    under = collections.Counter()
    adaptive = []
    for e in walk:
        for t in e["transitions"]:
            for k, v in t.get("update_under", {}).items():
                under[k] += bool(v)
            if "adaptive_verified" in t:
                adaptive.append(t)
    assert under["iso_and_skipping"] >= 1 and under["cached"] >= 1, under
    # ADAPTIVE retires at even frames: three frames behind its commit pass frame 2
    assert adaptive and all(t["frames"] == 3 and t["checks"][-1]["frame_index"] == 3 and t["state"]["accumulate"] for t in adaptive)
    assert sum(t["adaptive_verified"] for t in adaptive) >= 2


def test_adaptive_thresholds_retire_some_blocks_and_not_all(walk, ovr, oracle):
    """the thresholds derived from a definition: in the convergence model some but not all of the estimated blocks retire after frame 2"""
    M = ovr.convergence
    seen = 0
    for e in walk:
        for t in e["transitions"]:
            if not t.get("adaptive_verified"):
                continue
            s = dict(t["state"], convergence=(W.OFF, 0.0), accumulate=False)
            if W.frame_kind(s) == "march":
                frames = [W.march_definition(ovr, oracle, s, k)[0] for k in (1, 2, 3)]
            else:
                frames = [W.model_definition(ovr, s, k)[0] for k in (1, 2, 3)]
            n_b, E_b, _ = M.retirement_frames([np.nan_to_num(f) for f in frames], t["state"]["convergence"][1])
            estimated = E_b > 0
            assert (n_b[estimated] == 2).any() and (n_b[estimated] == 0).any(), (W.describe(t), n_b)
            seen += 1
    assert seen >= 2


def test_frame_index_model_agrees_with_the_commit_walk():
    """tests/commit_walk.py's literals, for the sources both know: its table is imported, not copied"""
    class Table:   # Walk.steps() builds closures over the setters and calls none of them
        base_layout, base_pipeline = -1, 0

        def __getattr__(self, name):
            return lambda *a, **k: (lambda: None)

    names = {"framebuffer": "fbsize", "camera": "camera", "transfer function": "tf", "focus": "focus", "spp": "spp", "sparse sampling": "sparse", "accumulation": "accumulation",
             "sampling rate": "rate", "shading": "shading", "jitter": "jitter", "convergence": "convergence", "reconstruction": "reconstruction", "image shard": "shard",
             "light": "light", "material": "material", "clip box": "clip", "shadow": "shadow", "LDS staging": "lds", "layout choice": "layout", "pipeline": "pipeline",
             "skipping": "skipping", "volume upload": "upload", "volume update": "update", "noise tile": "noise"}
    steps = commit_walk.Walk.steps(Table())
    idx = W.IndexModel(True)
    known = 0
    for step in steps:
        name, index = step[0], step[2]
        source = next((v for k, v in sorted(names.items(), key=lambda kv: -len(kv[0])) if name.startswith(k)), None)
        if len(step) < 5 or step[4]:   # the walk's own prelude: the camera set to what it is, three frames
            idx.call("camera", False)
            for _ in range(3):
                idx.render()
            assert idx.index == 3
        if source is None:
            assert name.startswith("grid convention"), name
            idx.call("camera", False)   # (a source this walk does not know: it starts over there)
        else:
            idx.call(source, not name.endswith("same"))
            if source == "accumulation":
                idx.accumulate = "(off)" not in name
            known += 1
        assert idx.render() == index or source is None, (name, idx.index, index)
    assert known >= 70
    # the frame-kind setters are recorded with the shading mode (csrc/ovr_hip_api.cpp consume_queued): EVERY call starts over
    assert W.starts_over("projection", False) and W.starts_over("isosurfaces", False) and W.starts_over("shading", False)


def _hits(ovr, s, frame_index):
    rgba, layer, cnt = W.model_definition(ovr, s, frame_index)
    return rgba, layer, int((layer[..., 2] > 0).sum())


def test_every_drawn_state_draws_something(walk, ovr):
    """the floor of the feature tests: more than 40 hit pixels in the model frame of every checked projection or isosurface state; all zeros under the empty box"""
    seen, empty = set(), 0
    counts = collections.Counter()
    for e, t, c in _checked(walk):
        s = t["state"]
        if t["kind"] == "march":
            continue
        key = repr(sorted((k, v) for k, v in s.items() if k not in ("accumulate", "convergence", "sparse", "focus", "reconstruction", "shard", "layout", "pipeline", "lds", "shadow", "spp", "jitter")))
        if key in seen:
            continue
        seen.add(key)
        plain = dict(s, spp=1, jitter=0)   # (the pixel centres: what is in view does not depend on the jitter)
        rgba, layer, hits = _hits(ovr, plain, 1)
        if s["clip"] == W.CLIP_EMPTY:
            assert not rgba.any() and not layer.any(), W.describe(t)
            empty += 1
        else:
            assert hits > 40, (hits, W.describe(t))
        counts[t["kind"]] += 1
    assert empty >= 1
    print(f"distinct drawn states per kind {dict(counts)}, under the empty box {empty}")
