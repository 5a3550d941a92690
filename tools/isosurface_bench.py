#!/usr/bin/env python3
"""isosurface_bench.py - what the isosurfaces (include/ovr_hip.h: ovr_hip_set_isosurfaces) cost on the MI355X.

tools/projection_bench.py's protocol: bench.py's c3 shape (1024^3 f32, 1920 x 1080) and c2 shape (512^3 f32, 1024 x 1024); per configuration every state is a
renderer of its own in ONE process, measured ALTERNATED in blocks of `--frames` frames, `--blocks` times each, after `--settle` untimed frames.  States:

  march         the unshaded march (OVR_HIP_SHADE_NONE) under an ALL-ZERO alpha table, skipping off, the general layout forced: every step of every ray
  maximum+rs    ovr_hip_set_projection(MAXIMUM) with range skipping
  iso/<shading>[+rs]/<level>   the isosurface frame under NONE, GRADIENT and FULL shading, without and with range skipping, for the level `through` (an isovalue
                through the synthetic blob, --through) and the level `miss` (an isovalue above every voxel, --miss: no ray hits, every ray walks to its end)

`--parent-tree DIR` (a built checkout of the parent commit) measures march and maximum+rs there, in a child process, before anything else.  Both are kernels
this change does not touch: the tool reports whether their medians here lie within the parent's block-to-block spread of the parent's.
Reported per state: min / median / max over the blocks of the per-block mean kernel_ms (device events around the frame's kernels), steps walked (samples +
skipped_samples), steps skipped, hits (shaded_samples), shadow steps.  The tool ASSERTS that a state with range skipping walks the steps and finds the hits of
its twin without, and that a `miss` level walks the march's steps.  One JSON line per configuration on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c3": dict(n=1024, width=1920, height=1080), "c2": dict(n=512, width=1024, height=1024)}

# march and maximum+rs alone, for a tree that does not know the isosurfaces: run with cwd = the tree, prints one JSON line
PARENT_CHILD = r'''
import json, sys
sys.path.insert(0, ".")
import numpy as np, torch
import ovr_amd as ovr
n, w, h, settle, frames, blocks = (int(x) for x in sys.argv[1:7])
dev = torch.device("cuda", 0)
vol = ovr.synth.make_volume_torch(n, dev, "float32")
cam = ovr.synth.make_camera("oblique", n)
def make(projection, skipping):
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    if not projection:
        alphas = np.array(alphas, np.float32); alphas[1::2] = 0.0
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((w, h)); ren.set_frame_accumulation(True); ren.set_shading(0); ren.set_layout_choice(0); ren.set_empty_space_skipping(skipping)
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam); ren.set_sparse_sampling(False)
    if projection: ren.set_projection(projection)
    ren.commit()
    return ren
rens = {"march": make(0, False), "maximum+rs": make(1, True)}
for ren in rens.values():
    for _ in range(settle): ren.render()
rows = {k: [] for k in rens}
for _ in range(blocks):
    for k, ren in rens.items():
        t = 0.0
        for _ in range(frames):
            ren.render(); t += ren.stats().kernel_ms
        rows[k].append(t / frames)
print(json.dumps({k: dict(kernel_ms=rows[k], samples=int(rens[k].stats().samples), skipped=int(rens[k].stats().skipped_samples)) for k in rens}))
'''


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def parent_states(args, shape):
    if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "open-volume-renderer_amd")):
        return None
    env = dict(os.environ)
    env.pop("OVR_HIP_LIBRARY", None)
    out = subprocess.run([sys.executable, "-c", PARENT_CHILD] + [str(shape[k]) for k in ("n", "width", "height")] + [str(args.settle), str(args.frames), str(args.blocks)],
                         cwd=args.parent_tree, env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        return dict(error=(out.stdout + out.stderr)[-600:])
    rec = json.loads(lines[-1])
    return {k: dict(kernel_ms=spread(v["kernel_ms"]), steps=v["samples"] + v["skipped"], skipped=v["skipped"]) for k, v in rec.items()}


def make_renderer(ctx, shape, vol, shading=0, skipping=False, projection=0, iso=None):
    ovr, torch, np = ctx
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    if projection == 0 and iso is None:
        alphas = np.array(alphas, np.float32)
        alphas[1::2] = 0.0
    cam = ovr.synth.make_camera("oblique", shape["n"])
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((shape["width"], shape["height"]))
    ren.set_frame_accumulation(True)
    ren.set_shading(shading)
    ren.set_layout_choice(0)
    ren.set_empty_space_skipping(skipping)
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam)
    ren.set_sparse_sampling(False)
    if projection:
        ren.set_projection(projection)
    if iso is not None:
        ren.set_isosurfaces([iso])
    ren.commit()
    return ren


def leg(ctx, args, name):
    ovr, torch, np = ctx
    shape = SHAPES[name]
    rec = dict(config=name, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, through=args.through, miss=args.miss)
    parent = parent_states(args, shape)   # a child process, before this process holds the volume
    if parent is not None:
        rec["parent"] = parent
    vol = ovr.synth.make_volume_torch(shape["n"], torch.device("cuda", 0), "float32")
    rens = {"march": make_renderer(ctx, shape, vol), "maximum+rs": make_renderer(ctx, shape, vol, skipping=True, projection=ovr.PROJECT_MAXIMUM)}
    for level, iso in (("through", args.through), ("miss", args.miss)):
        for sname, shading in (("none", 0), ("gradient", 1), ("full", 2)):
            for rs in (False, True):
                rens[f"iso/{sname}{'+rs' if rs else ''}/{level}"] = make_renderer(ctx, shape, vol, shading=shading, skipping=rs, iso=iso)
    del vol
    torch.cuda.empty_cache()
    for ren in rens.values():
        for _ in range(args.settle):
            ren.render()
    rows = {k: [] for k in rens}
    for _ in range(args.blocks):
        for k, ren in rens.items():
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[k].append(t / args.frames)
    st = {k: ren.stats() for k, ren in rens.items()}
    steps = int(st["march"].samples)
    assert st["march"].layout == 0 and st["march"].skipped_samples == 0
    for k, s in st.items():
        rec[k] = dict(kernel_ms=spread(rows[k]), steps=int(s.samples + s.skipped_samples), skipped=int(s.skipped_samples), hits=int(s.shaded_samples),
                      shadow_steps=int(s.shadow_samples + s.skipped_shadow_samples), shadow_skipped=int(s.skipped_shadow_samples))
        if k.startswith("iso/") and "+rs" in k:
            twin = rec[k.replace("+rs", "")]
            assert rec[k]["steps"] == twin["steps"] and rec[k]["hits"] == twin["hits"] and rec[k]["shadow_steps"] == twin["shadow_steps"], (k, rec[k], twin)
            assert rens[k].get_isosurfaces().range_skipping == 1
        if k.endswith("/miss"):
            assert rec[k]["steps"] == steps and rec[k]["hits"] == 0, (k, rec[k], steps)
    assert rec["maximum+rs"]["steps"] == steps
    if parent is not None and "error" not in parent:
        assert parent["march"]["steps"] == steps and parent["maximum+rs"]["steps"] == steps and parent["maximum+rs"]["skipped"] == rec["maximum+rs"]["skipped"]
        for k in ("march", "maximum+rs"):
            p, h = parent[k]["kernel_ms"], rec[k]["kernel_ms"]
            rec[k]["vs_parent_ms"] = round(h["median"] - p["median"], 4)
            rec[k]["parent_spread_ms"] = round(p["max"] - p["min"], 4)
            rec[k]["within_parent_spread"] = bool(abs(h["median"] - p["median"]) <= max(p["max"] - p["min"], h["max"] - h["min"]))
    for ren in rens.values():
        ren.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("configs", nargs="*", default=["c3", "c2"], choices=sorted(SHAPES))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--frames", type=int, default=40, help="frames per timed block")
    ap.add_argument("--settle", type=int, default=20, help="untimed frames per state before the first block")
    ap.add_argument("--blocks", type=int, default=5, help="how often every state is measured, alternated")
    ap.add_argument("--through", type=float, default=0.5, help="the isovalue through the synthetic blob")
    ap.add_argument("--miss", type=float, default=2.0, help="an isovalue no voxel reaches")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("isosurface_bench.py needs an MI355X")
    lines = []
    for name in args.configs:
        lines.append(json.dumps(leg((ovr, torch, np), args, name)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
