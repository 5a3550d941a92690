"""The launches the unsigned voxel types miss elsewhere in the suite.

1. uint16 and uint8 under the aligned 8-byte row loads (addressing mode 4; OVR_HIP_ROW_LOADS=1 - by size it takes a layout above 128 MiB) in everything but the
   plain march: the four known-answer entries against the models, one frame each of projection maximum, opaque isosurface, translucent isosurface and ambient
   occlusion, and a clipped, an orthographic, a lit and a cached march in both pipelines.  Every frame is bit-identical, counters included, to the same frame
   with OVR_HIP_ROW_LOADS=0, and is checked against its definition once.  The bodies are tests/test_signed_types_gpu.py's, with the voxel type as a parameter.
2. The shadow cache under the addressing modes 1, 2, 3 (float32, uint16, int16) and the row loads (the 16-bit types): the bodies of
   test_shadow_cache_gpu.test_nodes_vs_oracle and test_shadow_floats_march_vs_oracle at their bars; the lattice read back equals mode 0's bit for bit, and a cached
   frame in each pipeline equals mode 0's, counters included.

The library reports no addressing mode: tests/launch_plan_driver.cpp pins OVR_HIP_ROW_LOADS -> mode 4 and OVR_HIP_ADDRESSING -> the mode, signed_cases.set_addressing
sets the variables before a renderer exists, and profiles/r21_signed_and_row_loads.md lists the instantiations a kernel trace of this file saw dispatched."""
import numpy as np
import pytest

import signed_cases as SC
import test_shadow_cache_gpu as TS
import test_signed_types_gpu as G
from helpers import hip_setup

pytestmark = pytest.mark.gpu
F = np.float32
UNSIGNED = (np.uint16, np.uint8)
IDS = lambda d: np.dtype(d).name
_memo = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _identical(rows, plain, name):
    assert len(rows) == len(plain) > 0, name
    for k, (a, b) in enumerate(zip(rows, plain)):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), (name, k, "the frame differs from the one without row loads")
        assert a[2] == b[2], (name, k, "counters", a[2], b[2])


# ---- 1. uint16 and uint8 under the row loads -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", UNSIGNED, ids=IDS)
@pytest.mark.parametrize("entry", ("project", "isosurface", "layer", "ao"))
def test_known_answer_entries_under_row_loads(ovr, hip_renderer_factory, monkeypatch, entry, dtype):
    SC.set_addressing(monkeypatch, "rows")
    body = {"project": G.project_floats_body, "isosurface": G.isosurface_floats_body, "layer": G.layer_floats_body, "ao": G.ao_floats_body}[entry]
    body(ovr, hip_renderer_factory, dtype, "rows")


FRAMES = {
    "maximum": lambda ovr, oracle, make, dtype, check: G.projection_frames_body(ovr, oracle, make, dtype, modes=(G.MAXIMUM,), check=check),
    "isosurface": lambda ovr, oracle, make, dtype, check: G.isosurface_frames_body(ovr, oracle, make, dtype, sets=("edge",), shadings=(2,), check=check),
    "translucent": G.translucent_frame_body,
    "ao": G.ao_frame_body,
    "clipped march": G.clipped_march_body,
    "orthographic march": G.orthographic_march_body,
    "lit march": G.lit_march_body,
    "cached march": G.cached_march_body,
}


@pytest.mark.parametrize("dtype", UNSIGNED, ids=IDS)
@pytest.mark.parametrize("frame", list(FRAMES), ids=lambda s: s.replace(" ", "_"))
def test_frames_under_row_loads(ovr, oracle, hip_renderer_factory, monkeypatch, frame, dtype):
    SC.set_addressing(monkeypatch, "rows")
    rows = FRAMES[frame](ovr, oracle, hip_renderer_factory, dtype, True)        # against its definition, once
    SC.set_addressing(monkeypatch, "no rows")
    plain = FRAMES[frame](ovr, oracle, hip_renderer_factory, dtype, False)
    _identical(rows, plain, (frame, np.dtype(dtype).name))
    if frame == "cached march":
        assert all(np.array_equal(_bits(a[3]), _bits(b[3])) for a, b in zip(rows, plain)), "the lattice differs from the one built without row loads"


# ---- 2. the shadow cache under every addressing mode ----------------------------------------------------------------------------------------------------

CACHE_CASES = [(dtype, am) for dtype in (np.float32, np.uint16, np.int16) for am in (1, 2, 3) + (("rows",) if np.dtype(dtype).itemsize == 2 else ())]


def _cache_run(ovr, oracle, make, dtype, check):
    """what one addressing mode gives: the lattice, the hook's marched shadow terms and a cached frame per pipeline"""
    name = np.dtype(dtype).name
    case = TS._case(ovr, oracle, dtype=dtype, tf="sparse")
    if check:       # the body of test_nodes_vs_oracle
        ren = make()
        TS.nodes_vs_oracle(ovr, oracle, ren, case, 4, f"nodes {name}")
        ren.close()
    # the body of test_shadow_floats_march_vs_oracle (the oracle's values once per type)
    ren = hip_setup(ovr, make(), case)
    pos = TS._positions(np.random.default_rng(21), 2000, case)
    marched = ren.shadow_floats(pos, 0)
    if check:
        key = ("shadow floats", name)
        if key not in _memo:
            _memo[key] = TS.oracle_shadow(ovr, oracle, case, np.array(list(ren.lighting().direction), F), pos)[0]
        want = _memo[key]
        assert (want > 0).sum() > 50 and (want == 0).sum() > 0
        TS.check_values(f"shadow_floats which 0, {name}", marched, want)
    assert ren.shadow_cache().builds == 0
    ren.close()
    frames = []
    for pipeline in (1, 2):
        ren = TS._cached(ovr, make(), case, cell=4, pipeline=pipeline)
        frame = TS._render(ovr, ren)
        lattice = ren.shadow_cache_values()
        assert ren.stats().pipeline == pipeline and ren.shadow_cache().builds == 1 and frame[2][3] == 0 and frame[2][2] > 0
        ren.close()
        frames.append(frame)
    return lattice, marched, frames


@pytest.mark.parametrize("dtype,am", CACHE_CASES, ids=lambda x: str(x) if isinstance(x, (int, str)) else np.dtype(x).name)
def test_shadow_cache_under_every_addressing_mode(ovr, oracle, hip_renderer_factory, monkeypatch, dtype, am):
    key = ("mode 0", np.dtype(dtype).name)
    if key not in _memo:
        SC.set_addressing(monkeypatch, 0)
        _memo[key] = _cache_run(ovr, oracle, hip_renderer_factory, dtype, False)
    SC.set_addressing(monkeypatch, am)
    lattice, marched, frames = _cache_run(ovr, oracle, hip_renderer_factory, dtype, True)
    base = _memo[key]
    assert lattice.max() > 0.1 and np.array_equal(_bits(lattice), _bits(base[0])), "the lattice differs from mode 0's"
    assert np.array_equal(_bits(marched), _bits(base[1])), "the hook's marched shadow terms differ from mode 0's"
    for pipeline, a, b in zip((1, 2), frames, base[2]):
        TS._same({"mode 0": b, str(am): a})
