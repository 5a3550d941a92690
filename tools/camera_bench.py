#!/usr/bin/env python3
"""camera_bench.py - what the orthographic camera (include/ovr_hip.h: ovr_hip_set_camera_orthographic) costs on the MI355X.

tools/isosurface_bench.py's protocol: bench.py's c3 shape (1024^3 f32, 1920 x 1080) and c2 shape (512^3 f32, 1024 x 1024); per configuration every state is a
renderer of its own in ONE process, measured ALTERNATED in blocks of `--frames` frames, `--blocks` times each, after `--settle` untimed frames.  States, each
for the views `oblique` and `axis` (the front view, where the thin replicas serve every ray of an orthographic frame):

  <kind>/perspective     the frame as it was: kind = march0 (unshaded march), march2 (full shading, the pooled pipeline where the tuner picks it), maximum+rs
                         (MAXIMUM with range skipping), iso (one isovalue, full shading, range skipping)
  <kind>/clipped         the same perspective frame with the volume's own box as the clip box: the clipped twin, the kernel the orthographic one is derived from
  <kind>/orthographic    the orthographic camera at the height that shows what the perspective camera shows at the plane through the volume's centre

`--parent-tree DIR` (a built checkout of the parent commit) measures the perspective states there, in a child process, before anything else - or, with
`--parent-last`, behind everything else, so that two runs separate the order of the processes from a real difference: kernels this change must not move.
`--variants perspective` measures here what is measured in the parent, and nothing else: two processes of the same composition.
`--kinds` / `--views` restrict the states: every state is a renderer with a resident volume of its own, and 24 of them do not fit at 1024^3.  The tool reports whether their medians here lie within the parent's block-to-block spread.
Reported per state: min / median / max over the blocks of the per-block mean kernel_ms (device events around the frame's kernels), steps walked (samples +
skipped_samples) and nanoseconds per step.  One JSON line per configuration on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c3": dict(n=1024, width=1920, height=1080), "c2": dict(n=512, width=1024, height=1024)}
KINDS = ("march0", "march2", "maximum+rs", "iso")

# the states of one tree: run with cwd = the tree, prints one JSON line.  argv: n w h settle frames blocks through variants(comma list)
CHILD = r'''
import json, math, sys
sys.path.insert(0, ".")
import numpy as np, torch
import ovr_amd as ovr
n, w, h, settle, frames, blocks = (int(x) for x in sys.argv[1:7])
through, variants, kinds, views = float(sys.argv[7]), sys.argv[8].split(","), sys.argv[9].split(","), sys.argv[10].split(",")
dev = torch.device("cuda", 0)
vol = ovr.synth.make_volume_torch(n, dev, "float32")
def make(kind, view, variant):
    cam = ovr.synth.make_camera("front" if view == "axis" else "oblique", n)
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    if kind == "march0":
        alphas = np.array(alphas, np.float32); alphas[1::2] = 0.0
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((w, h)); ren.set_frame_accumulation(True); ren.set_shading(0 if kind == "march0" else 2)
    ren.set_empty_space_skipping(kind != "march0")
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam); ren.set_sparse_sampling(False)
    if kind == "maximum+rs": ren.set_projection(1)
    if kind == "iso": ren.set_isosurfaces([through])
    if variant == "clipped": ren.set_clip_box((0.0, 0.0, 0.0), (float(n), float(n), float(n)))
    if variant == "orthographic":
        eye, at, up = cam
        ren.set_camera(ovr.Camera(eye, at, up, orthographic_height=ovr.camera.auto_height(eye, at, 60.0)))
    ren.commit()
    return ren
rens = {f"{k}/{v}/{x}": make(k, v, x) for k in kinds for v in views for x in variants}
for ren in rens.values():
    for _ in range(settle): ren.render()
rows = {k: [] for k in rens}
for _ in range(blocks):
    for k, ren in rens.items():
        t = 0.0
        for _ in range(frames):
            ren.render(); t += ren.stats().kernel_ms
        rows[k].append(t / frames)
out = {}
for k, ren in rens.items():
    st = ren.stats()
    out[k] = dict(kernel_ms=rows[k], samples=int(st.samples), skipped=int(st.skipped_samples), layout=int(st.layout), pipeline=int(st.pipeline))
print(json.dumps(out))
'''


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def run_tree(tree, args, shape, variants):
    env = dict(os.environ)
    env.pop("OVR_HIP_LIBRARY", None)
    out = subprocess.run([sys.executable, "-c", CHILD] + [str(shape[k]) for k in ("n", "width", "height")] + [str(args.settle), str(args.frames), str(args.blocks), str(args.through), variants, args.kinds, args.views],
                         cwd=tree, env=env, capture_output=True, text=True, timeout=1100)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        return dict(error=(out.stdout + out.stderr)[-600:])
    rec = {}
    for k, v in json.loads(lines[-1]).items():
        steps = v["samples"] + v["skipped"]
        s = spread(v["kernel_ms"])
        rec[k] = dict(kernel_ms=s, steps=steps, skipped=v["skipped"], ns_per_step=round(s["median"] * 1e6 / steps, 5) if steps else None, layout=v["layout"], pipeline=v["pipeline"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(SHAPES))
    ap.add_argument("--settle", type=int, default=6)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--through", type=float, default=0.5)
    ap.add_argument("--kinds", default=",".join(KINDS), help="comma list out of " + ",".join(KINDS))
    ap.add_argument("--views", default="oblique,axis")
    ap.add_argument("--variants", default="perspective,clipped,orthographic", help="of this tree; `perspective` alone makes this tree's process the parent's: the same states, the same number of resident volumes")
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-last", action="store_true", help="measure the parent tree BEHIND this one: separates the order of the two processes from a real difference")
    ap.add_argument("--out")
    args = ap.parse_args()
    shape = SHAPES[args.config]
    rec = dict(config=args.config, parent_last=bool(args.parent_last), **shape)
    have_parent = args.parent_tree and os.path.isdir(os.path.join(args.parent_tree, "open-volume-renderer_amd"))
    if have_parent and not args.parent_last:
        rec["parent"] = run_tree(args.parent_tree, args, shape, "perspective")
    rec["here"] = run_tree(ROOT, args, shape, args.variants)
    if have_parent and args.parent_last:
        rec["parent"] = run_tree(args.parent_tree, args, shape, "perspective")
    if "parent" in rec and "error" not in rec["parent"] and "error" not in rec["here"]:
        verdict = {}
        for k, p in rec["parent"].items():
            m = rec["here"][k]["kernel_ms"]["median"]
            verdict[k] = dict(parent=p["kernel_ms"], here=m, inside=p["kernel_ms"]["min"] <= m <= p["kernel_ms"]["max"])
        rec["existing_paths"] = verdict
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 1 if "error" in rec["here"] else 0


if __name__ == "__main__":
    sys.exit(main())
