"""The one path of the seven known-answer ray queries on the GPU (ovr_hip_api.cpp ray_query, ovr_hip_kernels.hip launch_ray_query, csrc/host/ray_query.hpp): every
entry refuses with its own message while something it needs is not committed, n = 0 touches nothing, and n = 5 writes exactly five records of the entry's size -
at max_events 1 and 16 as well as the 8 every other test uses: the size comes from the table, and a wrong one would show nowhere else.  A 40 x 33 x 18 u8 volume,
5 rays (20 lanes: less than one workgroup), `out` one record longer than needed and filled with NaN.  What the records hold is the business of each kind's own
known-answer test; the refusals a committed renderer cannot reach (no transfer function, no macrocell ranges) are tests/test_ray_query_table.py's."""
import numpy as np
import pytest

import isosurface_context_cases as XC
import projection_cases as PC
import slice_context_cases as CC
from helpers import hip_setup

pytestmark = pytest.mark.gpu
F = np.float32
N = 5
# entry -> (arguments behind (org, dir, out, n) as a function of max_events, header floats, floats per event, out is zeroed first)
ENTRIES = {
    "ovr_hip_project_floats": (lambda m: (1, 1), 4, 0, False),
    "ovr_hip_slice_floats": (lambda m: (1,), 4, 0, False),
    "ovr_hip_slice_context_floats": (lambda m: (), 8, 0, False),
    "ovr_hip_isosurface_floats": (lambda m: (1,), 8, 0, False),
    "ovr_hip_isosurface_layers_floats": (lambda m: (m, 1), 4, 8, True),
    "ovr_hip_isosurface_context_floats": (lambda m: (m,), 8, 8, True),
    "ovr_hip_isosurface_ao_floats": (lambda m: (m, 3, 1), 8, 8, True),
}


def _rays():
    """five rays at the ball in the middle of the volume: through its centre (events on both sides of both shells), off centre, grazing, and one past the box"""
    org = np.array([[20.0, 16.5, -60.0], [-30.0, 40.0, -35.0], [26.0, 19.0, -60.0], [31.0, 16.5, -60.0], [20.0, 80.0, -60.0]], F)
    at = np.array([[20.0, 16.5, 9.0], [20.0, 16.5, 9.0], [26.0, 19.0, 9.0], [31.0, 16.5, 9.0], [20.0, 80.0, 9.0]], F)
    d = at - org
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def _refused(lib, ren, buf, entry, message):
    p = buf.data_ptr()
    code = getattr(lib, entry)(ren._h, p, p, p, 1, *ENTRIES[entry][0](8))
    assert code == -3 and lib.ovr_hip_last_error() == f"[hip] {entry}: {message}".encode(), (entry, code, lib.ovr_hip_last_error())


def test_every_entry_on_the_one_path(ovr, hip_renderer_factory):
    import torch
    dev = torch.device("cuda", 0)
    lib = ovr._lib.load()
    buf = torch.zeros(160, dtype=torch.float32, device=dev)
    vol = XC.volume(np.uint8)
    assert vol.shape == (18, 33, 40)
    colors, alphas, vr = XC.transfer_function(ovr, "dense", np.uint8)
    case = dict(vol=vol, colors=colors, alphas=alphas, vr=vr, cam=PC.CAMERAS["axis"], size=PC.SIZE, shading=2, rate=1.0, spp=1, convention=0, spacing=(1.0, 1.0, 1.0),
                origin=(0.0, 0.0, 0.0), fovy=PC.FOVY)
    ren = hip_renderer_factory()
    # (a) the refusals, in the order the state is built up: ESTATE and the entry's own message
    for entry in ENTRIES:
        _refused(lib, ren, buf, entry, "no volume was set")
    hip_setup(ovr, ren, case)
    for entry, setter in (("ovr_hip_slice_floats", "ovr_hip_set_slices"), ("ovr_hip_slice_context_floats", "ovr_hip_set_slices")):
        _refused(lib, ren, buf, entry, f"no slice is committed ({setter})")
    for entry, setter in (("ovr_hip_isosurface_floats", "ovr_hip_set_isosurfaces"), ("ovr_hip_isosurface_layers_floats", "ovr_hip_set_isosurface_layers"),
                          ("ovr_hip_isosurface_context_floats", "ovr_hip_set_isosurfaces"), ("ovr_hip_isosurface_ao_floats", "ovr_hip_set_isosurface_layers")):
        _refused(lib, ren, buf, entry, f"no isovalue is committed ({setter})")
    ren.set_slices(CC.SLICES)
    ren.set_isosurfaces(XC.isovalues(XC.LEVELS, np.uint8), XC.SHELLS)
    ren.commit()
    _refused(lib, ren, buf, "ovr_hip_slice_context_floats", "no slice context is committed (ovr_hip_set_slice_context)")
    _refused(lib, ren, buf, "ovr_hip_isosurface_context_floats", "no isosurface context is committed (ovr_hip_set_isosurface_context)")
    _refused(lib, ren, buf, "ovr_hip_isosurface_ao_floats", "no ambient-occlusion sample is committed (ovr_hip_set_ambient_occlusion)")
    # everything committed at once: each query scrubs what is not its own
    ren.set_slice_context(1, 0.5)
    ren.set_isosurface_context(1, 0.5)
    ren.set_ambient_occlusion(4, 6.0)
    ren.commit()
    org, direction = (torch.from_numpy(a).to(dev) for a in _rays())
    for entry, (args, header, per_event, zeroed) in ENTRIES.items():
        for m in (1, 16) if per_event else (8,):
            width = header + per_event * m
            out = torch.full((N + 1, width), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            # (b) no rays: nothing is written
            assert getattr(lib, entry)(ren._h, org.data_ptr(), direction.data_ptr(), out.data_ptr(), 0, *args(m)) == 0, (entry, lib.ovr_hip_last_error())
            torch.cuda.synchronize(dev)
            assert bool(torch.isnan(out).all()), (entry, m, "n = 0 wrote")
            # (c) five rays: five finite records, zeros behind a ray's events, the sixth record untouched
            assert getattr(lib, entry)(ren._h, org.data_ptr(), direction.data_ptr(), out.data_ptr(), N, *args(m)) == 0, (entry, lib.ovr_hip_last_error())
            o = out.cpu().numpy()
            print(entry, m, o[:N, :header].tolist())
            assert np.isfinite(o[:N]).all(), (entry, m, o[:N])
            assert np.isnan(o[N]).all(), (entry, m, "the guard record was written", o[N])
            if zeroed:
                events = o[:N, 0].astype(np.int64)
                slots = o[:N, header:].reshape(N, m, per_event)
                assert events.max() >= 2 and events.min() == 0, (entry, events)     # a ray with more events than one slot, and a ray with none
                for i in range(N):
                    assert not slots[i, min(events[i], m):].any(), (entry, m, i, events[i], slots[i])
                    assert slots[i, :min(events[i], m), 1].all(), (entry, m, i, "an event without its t*")
    ren.close()
