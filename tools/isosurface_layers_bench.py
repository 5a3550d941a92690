#!/usr/bin/env python3
"""isosurface_layers_bench.py - what the translucent isosurfaces (include/ovr_hip.h: ovr_hip_set_isosurface_layers) cost on the MI355X.

tools/isosurface_bench.py's protocol: bench.py's c3 shape (1024^3 f32, 1920 x 1080) and c2 shape (512^3 f32, 1024 x 1024); per configuration every state is a
renderer of its own in ONE process, measured ALTERNATED in blocks of `--frames` frames, `--blocks` times each, after `--settle` untimed frames.  States:

  opaque/<n>/<shading>[+rs]        ovr_hip_set_isosurfaces with n = 2 and n = 4 nested isovalues (--two, --four) under NONE, GRADIENT and FULL shading, without and with
                                   range skipping: the first crossing
  translucent/<n>/<shading>[+rs]   the same isovalues through ovr_hip_set_isosurface_layers with the opacity --opacity each: every crossing composited

`--parent-tree DIR` (a built checkout of the parent commit) measures the opaque states there, in a child process, before anything else.  They are kernels this
change does not touch: the tool ASSERTS their steps, hits and shadow steps equal and reports whether their medians here lie within the parent's block-to-block
spread of the parent's.  Reported per state: min / median / max over the blocks of the per-block mean kernel_ms (device events around the frame's kernels), steps
walked (samples + skipped_samples), steps skipped, events (shaded_samples), shadow steps.  The tool ASSERTS that a state with range skipping walks the steps,
composites the events and walks the shadow steps of its twin without, and that the three shading modes of a level set walk the same steps and composite the same
events.  Per translucent state it derives us_per_extra_event = (its median - the opaque twin's) / (its events - the twin's hits), and per FULL state
us_per_shadow_walk = (its median - the GRADIENT twin's) / events.  One JSON line per configuration on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c3": dict(n=1024, width=1920, height=1080), "c2": dict(n=512, width=1024, height=1024)}
SHADINGS = (("none", 0), ("gradient", 1), ("full", 2))

# the opaque states alone, for a tree that does not know the opacities: run with cwd = the tree, prints one JSON line
PARENT_CHILD = r'''
import json, sys
sys.path.insert(0, ".")
import numpy as np, torch
import ovr_amd as ovr
n, w, h, settle, frames, blocks = (int(x) for x in sys.argv[1:7])
levels, shadings = json.loads(sys.argv[7]), json.loads(sys.argv[8])
dev = torch.device("cuda", 0)
vol = ovr.synth.make_volume_torch(n, dev, "float32")
cam = ovr.synth.make_camera("oblique", n)
def make(iso, shading, skipping):
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((w, h)); ren.set_frame_accumulation(True); ren.set_shading(shading); ren.set_layout_choice(0); ren.set_empty_space_skipping(skipping)
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam); ren.set_sparse_sampling(False)
    ren.set_isosurfaces(iso)
    ren.commit()
    return ren
rens = {}
for name, iso in levels.items():
    for sname, shading in shadings:
        for rs in (False, True):
            rens["opaque/%s/%s%s" % (name, sname, "+rs" if rs else "")] = make(iso, shading, rs)
del vol
torch.cuda.empty_cache()
for ren in rens.values():
    for _ in range(settle): ren.render()
rows = {k: [] for k in rens}
for _ in range(blocks):
    for k, ren in rens.items():
        t = 0.0
        for _ in range(frames):
            ren.render(); t += ren.stats().kernel_ms
        rows[k].append(t / frames)
st = {k: r.stats() for k, r in rens.items()}
print(json.dumps({k: dict(kernel_ms=rows[k], steps=int(s.samples + s.skipped_samples), skipped=int(s.skipped_samples), events=int(s.shaded_samples),
                          shadow_steps=int(s.shadow_samples + s.skipped_shadow_samples)) for k, s in st.items()}))
'''


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def parent_states(args, shape, levels, shadings):
    if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "open-volume-renderer_amd")):
        return None
    env = dict(os.environ)
    env.pop("OVR_HIP_LIBRARY", None)
    out = subprocess.run([sys.executable, "-c", PARENT_CHILD] + [str(shape[k]) for k in ("n", "width", "height")] + [str(args.settle), str(args.frames), str(args.blocks), json.dumps(levels), json.dumps(shadings)],
                         cwd=args.parent_tree, env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        return dict(error=(out.stdout + out.stderr)[-600:])
    rec = json.loads(lines[-1])
    return {k: dict(v, kernel_ms=spread(v["kernel_ms"])) for k, v in rec.items()}


def make_renderer(ctx, shape, vol, iso, opacities, shading, skipping):
    ovr, torch, np = ctx
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
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
    ren.set_isosurfaces(iso, opacities)
    ren.commit()
    return ren


def leg(ctx, args, name):
    ovr, torch, np = ctx
    shape = SHAPES[name]
    levels = {"2": list(args.two), "4": list(args.four)}
    shadings = [x for x in SHADINGS if x[0] in args.shadings]
    rec = dict(config=name, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, levels=levels, opacity=args.opacity)
    parent = parent_states(args, shape, levels, shadings)   # a child process, before this process holds the volume
    if parent is not None:
        rec["parent"] = parent
    vol = ovr.synth.make_volume_torch(shape["n"], torch.device("cuda", 0), "float32")
    rens = {}
    for kind in ("opaque", "translucent"):
        for lname, iso in levels.items():
            for sname, shading in shadings:
                for rs in (False, True):
                    rens[f"{kind}/{lname}/{sname}{'+rs' if rs else ''}"] = make_renderer(ctx, shape, vol, iso, None if kind == "opaque" else [args.opacity] * len(iso), shading, rs)
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
    for k, ren in rens.items():
        s = ren.stats()
        rec[k] = dict(kernel_ms=spread(rows[k]), steps=int(s.samples + s.skipped_samples), skipped=int(s.skipped_samples), events=int(s.shaded_samples),
                      shadow_steps=int(s.shadow_samples + s.skipped_shadow_samples), shadow_skipped=int(s.skipped_shadow_samples))
        assert ren.get_isosurface_layers().translucent == (1 if k.startswith("translucent/") else 0), k
    for k in rens:
        kind, lname, mode = k.split("/")
        if "+rs" in mode:
            twin = rec[k.replace("+rs", "")]
            assert rec[k]["steps"] == twin["steps"] and rec[k]["events"] == twin["events"] and rec[k]["shadow_steps"] == twin["shadow_steps"], (k, rec[k], twin)
            assert rens[k].get_isosurface_layers().range_skipping == 1
        base = rec[f"{kind}/{lname}/none"]
        assert rec[k]["steps"] == base["steps"] and rec[k]["events"] == base["events"], (k, rec[k], base)
        if kind == "translucent":
            twin = rec[k.replace("translucent/", "opaque/")]
            extra = rec[k]["events"] - twin["events"]
            assert extra > 0 and rec[k]["steps"] >= twin["steps"], (k, rec[k], twin)
            rec[k]["us_per_extra_event"] = round(1e3 * (rec[k]["kernel_ms"]["median"] - twin["kernel_ms"]["median"]) / extra, 6)
        if mode.startswith("full") and "gradient" in args.shadings:
            g = rec[k.replace("/full", "/gradient")]
            rec[k]["us_per_shadow_walk"] = round(1e3 * (rec[k]["kernel_ms"]["median"] - g["kernel_ms"]["median"]) / rec[k]["events"], 6)
    if parent is not None and "error" not in parent:
        for k, p in parent.items():
            assert p["steps"] == rec[k]["steps"] and p["events"] == rec[k]["events"] and p["shadow_steps"] == rec[k]["shadow_steps"] and p["skipped"] == rec[k]["skipped"], (k, p, rec[k])
            pm, hm = p["kernel_ms"], rec[k]["kernel_ms"]
            rec[k]["vs_parent_ms"] = round(hm["median"] - pm["median"], 4)
            rec[k]["parent_spread_ms"] = round(pm["max"] - pm["min"], 4)
            rec[k]["within_parent_spread"] = bool(abs(hm["median"] - pm["median"]) <= max(pm["max"] - pm["min"], hm["max"] - hm["min"]))
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
    ap.add_argument("--two", type=float, nargs=2, default=(0.35, 0.6), help="two nested isovalues of the synthetic blob")
    ap.add_argument("--four", type=float, nargs=4, default=(0.2, 0.35, 0.5, 0.65), help="four nested isovalues of the synthetic blob")
    ap.add_argument("--opacity", type=float, default=0.3, help="the opacity of every level of a translucent state")
    ap.add_argument("--shadings", nargs="+", default=["none", "gradient", "full"], choices=["none", "gradient", "full"], help="the shading modes measured (`none` is always needed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("isosurface_layers_bench.py needs an MI355X")
    lines = []
    for name in args.configs:
        lines.append(json.dumps(leg((ovr, torch, np), args, name)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
