#!/usr/bin/env python3
"""launch_states.py - one 96 x 64 frame of a 24^3 volume per named state, one state per kernel variant rule of csrc/host/launch_plan.hpp (24^3 spans
two macrocells per axis: the skipping kernels have work).  Every variant renders the same frame, so what a state LAUNCHES is only visible from outside:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_states.py

once with this tree's library and once with another build's (OVR_HIP_LIBRARY=...), then `python tools/launch_states.py --compare DIR_A DIR_B`: the two
traces must agree line for line, in dispatch order, on kernel name, grid size, workgroup size and LDS size.  Prints nothing but the state names."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INF = float("inf")
N, SIZE = 24, (96, 64)

# name -> (environment, settings): dtype, shading, pipeline (1 in place, 2 pooled), skip, material, clip, spp, shard, sparse, lds, layout, projection (mode),
# iso (isovalues of a [0, 1] field) with opacities, ortho, cache (the shadow cache: its build, then a cached frame), query (a known-answer entry, 8 rays),
# light, jitter (blue noise), convergence (mode, threshold), reconstruction (mode), frames (accumulated frames rendered: 1, two for a sparse state)
STATES = [
    ("unshaded_f32_lds_staged", {}, dict(shading=0, lds=True)),
    ("unshaded_f32_plain", {}, dict(shading=0, lds=False)),
    ("unshaded_f32_clipped", {}, dict(shading=0, lds=True, clip=True)),
]
for _s in (1, 2):
    STATES += [
        (f"shading{_s}_inplace_reference_material", {}, dict(shading=_s, pipeline=1)),
        (f"shading{_s}_inplace_other_material", {}, dict(shading=_s, pipeline=1, material=True)),
        (f"shading{_s}_inplace_clipped", {}, dict(shading=_s, pipeline=1, clip=True)),
        (f"shading{_s}_pooled", {}, dict(shading=_s, pipeline=2)),
        (f"shading{_s}_pooled_skipping", {}, dict(shading=_s, pipeline=2, skip=True)),
        (f"shading{_s}_pooled_other_material", {}, dict(shading=_s, pipeline=2, material=True)),
        (f"shading{_s}_pooled_clipped", {}, dict(shading=_s, pipeline=2, clip=True)),
        (f"shading{_s}_pooled_skipping_clipped", {}, dict(shading=_s, pipeline=2, skip=True, clip=True)),
        (f"shading{_s}_pooled_spp2", {}, dict(shading=_s, pipeline=2, spp=2)),
    ]
STATES += [
    ("shard_rank0_of_2_pooled", {}, dict(shading=2, pipeline=2, shard=(0, 2))),
    ("sparse_after_sparse", {}, dict(shading=2, pipeline=2, sparse=True)),
    ("addressing1", {"OVR_HIP_ADDRESSING": "1"}, dict(shading=2, pipeline=2)),
    ("addressing2", {"OVR_HIP_ADDRESSING": "2"}, dict(shading=2, pipeline=2)),
    ("addressing3", {"OVR_HIP_ADDRESSING": "3"}, dict(shading=2, pipeline=2)),
    ("addressing1_unshaded_lds_staged", {"OVR_HIP_ADDRESSING": "1"}, dict(shading=0, lds=True)),
    ("addressing2_unshaded", {"OVR_HIP_ADDRESSING": "2"}, dict(shading=0, lds=True)),
    ("u16_general", {}, dict(dtype="uint16", shading=2, pipeline=2)),
    ("u8_general", {}, dict(dtype="uint8", shading=2, pipeline=2)),
    ("u16_row_loads", {"OVR_HIP_ROW_LOADS": "1"}, dict(dtype="uint16", shading=2, pipeline=2)),
    ("u16_row_loads_addressing1", {"OVR_HIP_ROW_LOADS": "1", "OVR_HIP_ADDRESSING": "1"}, dict(dtype="uint16", shading=2, pipeline=2)),
    ("u16_row_loads_shard", {"OVR_HIP_ROW_LOADS": "1"}, dict(dtype="uint16", shading=2, pipeline=2, shard=(0, 2))),
    ("f32_thin_layout", {}, dict(shading=2, pipeline=2, layout=1)),
    ("u16_quad_layout", {}, dict(dtype="uint16", shading=2, pipeline=1, layout=3)),
]
ISO, LAYERS = (0.4, 0.6), dict(iso=(0.4, 0.6), opacities=(0.5, 1.0))
U16_ROWS = {"OVR_HIP_ROW_LOADS": "1"}
STATES += [
    ("projection_maximum", {}, dict(shading=0, projection=1)),
    ("projection_minimum", {}, dict(shading=0, projection=2)),
    ("projection_mean", {}, dict(shading=0, projection=3)),
    ("projection_maximum_range_skipping", {}, dict(shading=0, projection=1, skip=True)),
    ("projection_mean_skipping_on", {}, dict(shading=0, projection=3, skip=True)),
    ("projection_maximum_clipped", {}, dict(shading=0, projection=1, clip=True)),
    ("projection_maximum_orthographic", {}, dict(shading=0, projection=1, ortho=True)),
    ("projection_minimum_range_skipping_orthographic_clipped", {}, dict(shading=0, projection=2, skip=True, ortho=True, clip=True)),
    ("projection_u16_row_loads", U16_ROWS, dict(dtype="uint16", shading=0, projection=1)),
]
STATES += [(f"projection_addressing{_a}", {"OVR_HIP_ADDRESSING": str(_a)}, dict(shading=0, projection=1)) for _a in (1, 2, 3)]
STATES += [(f"isosurface_shading{_s}", {}, dict(shading=_s, iso=ISO)) for _s in (0, 1, 2)]
STATES += [
    ("isosurface_range_skipping", {}, dict(shading=2, iso=ISO, skip=True)),
    ("isosurface_clipped", {}, dict(shading=2, iso=ISO, clip=True)),
    ("isosurface_orthographic", {}, dict(shading=2, iso=ISO, ortho=True)),
    ("isosurface_range_skipping_orthographic", {}, dict(shading=1, iso=ISO, skip=True, ortho=True)),
    ("isosurface_u8", {}, dict(dtype="uint8", shading=2, iso=ISO)),
    ("isosurface_u16_row_loads", U16_ROWS, dict(dtype="uint16", shading=2, iso=ISO)),
    ("isosurface_addressing3", {"OVR_HIP_ADDRESSING": "3"}, dict(shading=2, iso=ISO)),
    ("translucent_shading0", {}, dict(shading=0, **LAYERS)),
    ("translucent_shading2", {}, dict(shading=2, **LAYERS)),
    ("translucent_shading0_orthographic", {}, dict(shading=0, ortho=True, **LAYERS)),
    ("translucent_shading2_orthographic", {}, dict(shading=2, ortho=True, **LAYERS)),
    ("translucent_range_skipping", {}, dict(shading=2, skip=True, **LAYERS)),
    ("translucent_u16_row_loads_clipped", U16_ROWS, dict(dtype="uint16", shading=1, clip=True, **LAYERS)),
    ("orthographic_unshaded", {}, dict(shading=0, lds=True, ortho=True)),
    ("orthographic_shading2_inplace", {}, dict(shading=2, pipeline=1, ortho=True)),
    ("orthographic_shading2_pooled", {}, dict(shading=2, pipeline=2, ortho=True)),
    ("orthographic_shading1_pooled_skipping", {}, dict(shading=1, pipeline=2, skip=True, ortho=True)),
    ("shadow_cache_inplace", {}, dict(shading=2, pipeline=1, cache=True)),
    ("shadow_cache_pooled", {}, dict(shading=2, pipeline=2, cache=True)),
    ("shadow_cache_u16_row_loads_orthographic", U16_ROWS, dict(dtype="uint16", shading=2, pipeline=2, cache=True, ortho=True)),
    ("query_project_rays", {}, dict(shading=0, query="project")),
    ("query_project_rays_u16_row_loads", U16_ROWS, dict(dtype="uint16", shading=0, query="project")),
    ("query_isosurface_rays", {}, dict(shading=2, iso=ISO, query="isosurface")),
    ("query_isosurface_rays_addressing2", {"OVR_HIP_ADDRESSING": "2"}, dict(shading=2, iso=ISO, query="isosurface")),
    ("query_isosurface_layer_rays", {}, dict(shading=2, query="layers", **LAYERS)),
    ("query_shadow_floats", {}, dict(shading=2, pipeline=1, query="shadow")),
    ("query_shadow_floats_u8_addressing1", {"OVR_HIP_ADDRESSING": "1"}, dict(dtype="uint8", shading=2, pipeline=1, query="shadow")),
]
# the frame-shaping setters tests/mode_walk.py walks that had no state here: light (direction and intensity; `material` above is the material alone), the
# blue-noise jitter, the convergence modes (`frames` accumulated frames: the estimate runs on even frames, ADAPTIVE retires blocks behind frame 2) and the
# reconstruction of a sparse frame
STATES += [
    ("other_light_inplace", {}, dict(shading=2, pipeline=1, light=True)),
    ("other_light_pooled", {}, dict(shading=2, pipeline=2, light=True)),
    ("isosurface_other_light", {}, dict(shading=2, iso=ISO, light=True)),
    ("blue_noise_jitter", {}, dict(shading=2, pipeline=2, jitter=True)),
    ("projection_blue_noise_jitter_spp2", {}, dict(shading=0, projection=1, jitter=True, spp=2)),
    ("convergence_estimate", {}, dict(shading=2, pipeline=2, convergence=(1, 0.0), frames=2)),
    ("convergence_adaptive", {}, dict(shading=2, pipeline=2, convergence=(2, 0.0), frames=4)),
    ("translucent_convergence_adaptive", {}, dict(shading=2, convergence=(2, 0.0), frames=4, **LAYERS)),
    ("sparse_reconstruction_fill", {}, dict(shading=2, pipeline=2, sparse=True, reconstruction=1)),
    ("projection_sparse_reconstruction_fill", {}, dict(shading=0, projection=1, sparse=True, reconstruction=1)),
]
ENV_KEYS = ("OVR_HIP_ADDRESSING", "OVR_HIP_ROW_LOADS")


def run_state(ovr, np, name, env, s):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    dtype = np.dtype(s.get("dtype", "float32"))
    vol = ovr.synth.make_volume(N, dtype=dtype)
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 256)
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize(SIZE)
    ren.set_frame_accumulation(True)
    ren.set_transfer_function(colors, alphas, vr)
    ren.set_shading(s["shading"])
    ren.set_shading_pipeline(s.get("pipeline", 0))
    ren.set_empty_space_skipping(bool(s.get("skip", False)))
    ren.set_lds_staging(bool(s.get("lds", False)))
    ren.set_sample_per_pixel(s.get("spp", 1))
    if "layout" in s:
        ren.set_volume_layouts(2)
        ren.set_layout_choice(s["layout"])
    else:
        ren.set_volume_layouts(0)
        ren.set_layout_choice(0)
    if s.get("material"):
        ren.set_material(0.3, 0.6, 0.4, 12.0)
    if s.get("light"):
        ren.set_light_direction((0.3, 0.8, -0.52), 1.5)
    if s.get("jitter"):
        ren.set_noise_tile(ovr.synth.make_noise_tile(16))
        ren.set_pixel_jitter(1)
    if "convergence" in s:
        ren.set_convergence(*s["convergence"])
    if "reconstruction" in s:
        ren.set_reconstruction(s["reconstruction"])
    if s.get("sparse"):
        ren.set_noise_tile(ovr.synth.make_noise_tile(16))
        ren.set_focus((0.5, 0.45), 0.35, 0.15)
        ren.set_sparse_sampling(True)
    if s.get("shard"):
        ren.set_image_shard(*s["shard"])
    eye, at, up = ovr.synth.make_camera("oblique", N)
    ren.init(ovr.Scene(volume=vol, transfer_function=None), ovr.Camera(eye, at, up, orthographic_height=ovr.camera.auto_height(eye, at, 60.0) if s.get("ortho") else None))
    if s.get("clip"):
        ren.set_clip_box((-INF, -INF, -INF), (N / 2.0, INF, INF))
    if "projection" in s:
        ren.set_projection(s["projection"])
    if "iso" in s:  # (in the samples' units: the 16-bit types' are raw)
        ren.set_isosurfaces([v * (65535.0 if dtype == np.uint16 else 1.0) for v in s["iso"]], s.get("opacities"))
    if s.get("cache"):
        ren.set_shadow_cache(1)
    ren.commit()
    for _ in range(s.get("frames", 2 if s.get("sparse") else 1)):
        ren.render()
    if "query" in s:  # 8 rays from the eye into the volume (the entries take the last frame's parameters)
        org = np.tile(np.asarray(eye, np.float32), (8, 1))
        aim = np.asarray(at, np.float32) + np.linspace(-0.2 * N, 0.2 * N, 8, dtype=np.float32)[:, None] * np.asarray([1.0, 0.5, 0.25], np.float32)
        d = aim - org
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        if s["query"] == "project":
            for mode, rs in ((1, False), (2, False), (3, False), (1, True), (2, True), (3, True)):
                ren.project_rays(org, d, mode, range_skipping=rs)
        elif s["query"] == "isosurface":
            for rs in (False, True):
                ren.isosurface_rays(org, d, range_skipping=rs)
        elif s["query"] == "layers":
            for rs in (False, True):
                ren.isosurface_layer_rays(org, d, max_events=4, range_skipping=rs)
        else:
            ren.shadow_floats(aim, 0)
    ren.close()
    print(name, flush=True)


def trace_rows(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"{directory}: expected one *kernel_trace.csv, found {len(files)}")
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"],
             r["LDS_Block_Size"] if "LDS_Block_Size" in r else r["Group_Segment_Size"]) for r in rows]


def compare(a, b):
    ra, rb = trace_rows(a), trace_rows(b)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(ra, rb)) if x != y]
    for i, x, y in bad[:10]:
        print(f"dispatch {i}:\n  {x}\n  {y}")
    march = sum("raymarch_kernel" in r[0] for r in ra)
    print(f"{len(ra)} / {len(rb)} dispatches ({march} of raymarch_kernel, {len(set(r[0] for r in ra))} distinct kernels), {len(bad)} differ")
    return 0 if ra and len(ra) == len(rb) and not bad else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    os.environ["OVR_HIP_TUNE"] = "0"  # the rules alone: nothing a state launches depends on a measured time
    import numpy as np
    import ovr_amd as ovr
    for name, env, s in STATES:
        run_state(ovr, np, name, env, s)
    return 0


if __name__ == "__main__":
    sys.exit(main())
