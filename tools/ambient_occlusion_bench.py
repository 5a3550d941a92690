#!/usr/bin/env python3
"""ambient_occlusion_bench.py - what ambient occlusion of the isosurface frames (include/ovr_hip.h: ovr_hip_set_ambient_occlusion) costs on
the MI355X.

tools/isosurface_layers_bench.py's protocol: bench.py's c3 shape (1024^3 f32, 1920 x 1080) and c2 shape (512^3 f32, 1024 x 1024); per configuration every state is
a renderer of its own in ONE process, measured ALTERNATED in blocks of `--frames` frames, `--blocks` times each, after `--settle` untimed frames.  States:

  <kind>/<n>/<shading>[+rs]/k0        kind = opaque | translucent (opacity --opacity each), n = 2 or 4 nested isovalues (--levels), shading = gradient | full,
                                      without and with range skipping: the frame without ambient occlusion
  <kind>/<n>/<shading>[+rs]/k<K>r<R>  the same frame with K in --samples walks per event, cut at R voxels (--distances; inf: the whole box)

`--parent-tree DIR` (a built checkout of the parent commit) measures the k0 states there, in a child process, before anything else: kernels this change does not
touch.  The tool ASSERTS their steps, events and shadow steps equal and reports whether their medians here lie within the parent's block-to-block spread.
Reported per state: min / median / max over the blocks of the per-block mean kernel_ms (device events around the frame's kernels), steps walked, events
(shaded_samples), shadow + AO steps.  The tool ASSERTS that an AO state walks the primary steps and composites the events of its k0 twin, and that a state with
range skipping walks what its twin without walks.  Per AO state it derives ao_steps (its shadow + AO steps minus the twin's shadow steps), us_per_ao_walk =
(its median - the twin's) / (events * K) and ns_per_ao_step = (its median - the twin's) / ao_steps; per FULL k0 state us_per_shadow_walk as section 19 does,
against the GRADIENT twin.  One JSON line per configuration on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c3": dict(n=1024, width=1920, height=1080), "c2": dict(n=512, width=1024, height=1024)}
SHADINGS = {"gradient": 1, "full": 2}
LEVELS = {"2": (0.35, 0.6), "4": (0.2, 0.35, 0.5, 0.65)}

# the k0 states alone, for a tree that does not know the setter: run with cwd = the tree, prints one JSON line
PARENT_CHILD = r'''
import json, sys
sys.path.insert(0, ".")
import numpy as np, torch
import ovr_amd as ovr
n, w, h, settle, frames, blocks = (int(x) for x in sys.argv[1:7])
states = json.loads(sys.argv[7])
dev = torch.device("cuda", 0)
vol = ovr.synth.make_volume_torch(n, dev, "float32")
cam = ovr.synth.make_camera("oblique", n)
def make(iso, opacities, shading, skipping):
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((w, h)); ren.set_frame_accumulation(True); ren.set_shading(shading); ren.set_layout_choice(0); ren.set_empty_space_skipping(skipping)
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam); ren.set_sparse_sampling(False)
    ren.set_isosurfaces(iso, opacities)
    ren.commit()
    return ren
rens = {k: make(*v) for k, v in states.items()}
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
print(json.dumps({k: dict(kernel_ms=rows[k], steps=int(s.samples + s.skipped_samples), events=int(s.shaded_samples),
                          shadow_steps=int(s.shadow_samples + s.skipped_shadow_samples)) for k, s in st.items()}))
'''


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def parent_states(args, shape, states):
    if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "open-volume-renderer_amd")):
        return None
    env = dict(os.environ)
    env.pop("OVR_HIP_LIBRARY", None)
    out = subprocess.run([sys.executable, "-c", PARENT_CHILD] + [str(shape[k]) for k in ("n", "width", "height")] + [str(args.settle), str(args.frames), str(args.blocks), json.dumps(states)],
                         cwd=args.parent_tree, env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        return dict(error=(out.stdout + out.stderr)[-600:])
    return {k: dict(v, kernel_ms=spread(v["kernel_ms"])) for k, v in json.loads(lines[-1]).items()}


def make_renderer(ctx, shape, vol, iso, opacities, shading, skipping, ao):
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
    if ao:
        ren.set_ambient_occlusion(*ao)
    ren.commit()
    return ren


def leg(ctx, args, name):
    ovr, torch, np = ctx
    shape = SHAPES[name]
    rec = dict(config=name, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, opacity=args.opacity, samples=args.samples, distances=args.distances)
    base = {}
    for kind in args.kinds:
        for lname in args.levels:
            for sname in args.shadings:
                for rs in args.range_skipping:
                    iso = list(LEVELS[lname])
                    base[f"{kind}/{lname}/{sname}{'+rs' if rs else ''}"] = (iso, None if kind == "opaque" else [args.opacity] * len(iso), SHADINGS[sname], bool(rs))
    parent = parent_states(args, shape, {k + "/k0": v for k, v in base.items()})   # a child process, before this process holds the volume
    if parent is not None:
        rec["parent"] = parent
    vol = ovr.synth.make_volume_torch(shape["n"], torch.device("cuda", 0), "float32")
    rens, ao_of = {}, {}
    for k, v in base.items():
        rens[k + "/k0"] = make_renderer(ctx, shape, vol, *v, None)
        for K in args.samples:
            for R in args.distances:
                key = f"{k}/k{K}r{R:g}"
                rens[key], ao_of[key] = make_renderer(ctx, shape, vol, *v, (K, R)), (K, k + "/k0")
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
        assert ren.get_ambient_occlusion().active == (1 if k in ao_of else 0), k
    for k in rens:
        if "+rs/" in k:
            twin = rec[k.replace("+rs/", "/")] if k.replace("+rs/", "/") in rec else None
            if twin is not None:
                assert rec[k]["steps"] == twin["steps"] and rec[k]["events"] == twin["events"] and rec[k]["shadow_steps"] == twin["shadow_steps"], (k, rec[k], twin)
        if k in ao_of:
            K, tk = ao_of[k]
            twin = rec[tk]
            assert rec[k]["steps"] == twin["steps"] and rec[k]["events"] == twin["events"] and rec[k]["shadow_steps"] >= twin["shadow_steps"], (k, rec[k], twin)
            d_ms = rec[k]["kernel_ms"]["median"] - twin["kernel_ms"]["median"]
            rec[k]["ao_steps"] = rec[k]["shadow_steps"] - twin["shadow_steps"]
            rec[k]["us_per_ao_walk"] = round(1e3 * d_ms / max(rec[k]["events"] * K, 1), 6)
            rec[k]["ns_per_ao_step"] = round(1e6 * d_ms / max(rec[k]["ao_steps"], 1), 6)
        elif "/full" in k and k.replace("/full", "/gradient") in rec:
            g = rec[k.replace("/full", "/gradient")]
            rec[k]["us_per_shadow_walk"] = round(1e3 * (rec[k]["kernel_ms"]["median"] - g["kernel_ms"]["median"]) / max(rec[k]["events"], 1), 6)
            rec[k]["ns_per_shadow_step"] = round(1e6 * (rec[k]["kernel_ms"]["median"] - g["kernel_ms"]["median"]) / max(rec[k]["shadow_steps"], 1), 6)
    if parent is not None and "error" not in parent:
        for k, p in parent.items():
            assert p["steps"] == rec[k]["steps"] and p["events"] == rec[k]["events"] and p["shadow_steps"] == rec[k]["shadow_steps"], (k, p, rec[k])
            pm, hm = p["kernel_ms"], rec[k]["kernel_ms"]
            rec[k]["vs_parent_ms"] = round(hm["median"] - pm["median"], 4)
            rec[k]["parent_spread_ms"] = round(pm["max"] - pm["min"], 4)
            rec[k]["within_parent_spread"] = bool(abs(hm["median"] - pm["median"]) <= max(pm["max"] - pm["min"], hm["max"] - hm["min"]))
    for ren in rens.values():
        ren.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("configs", nargs="*", default=["c2"], choices=sorted(SHAPES))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--frames", type=int, default=10, help="frames per timed block")
    ap.add_argument("--settle", type=int, default=3, help="untimed frames per state before the first block")
    ap.add_argument("--blocks", type=int, default=3, help="how often every state is measured, alternated")
    ap.add_argument("--samples", type=int, nargs="*", default=[4, 8, 16], help="K (none: the k0 states alone - like for like with the parent's process)")
    ap.add_argument("--distances", type=float, nargs="+", default=[8.0, float("inf")], help="R in voxels (the synthetic volume's spacing is 1)")
    ap.add_argument("--kinds", nargs="+", default=["opaque", "translucent"], choices=["opaque", "translucent"])
    ap.add_argument("--levels", nargs="+", default=["2", "4"], choices=sorted(LEVELS), help="section 17's / 19's two configurations: 2 or 4 nested isovalues")
    ap.add_argument("--shadings", nargs="+", default=["gradient", "full"], choices=sorted(SHADINGS))
    ap.add_argument("--range-skipping", type=int, nargs="+", default=[0, 1], choices=[0, 1])
    ap.add_argument("--opacity", type=float, default=0.3, help="the opacity of every level of a translucent state")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("ambient_occlusion_bench.py needs an MI355X")
    lines = []
    for name in args.configs:
        lines.append(json.dumps(leg((ovr, torch, np), args, name)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
