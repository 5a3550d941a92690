#!/usr/bin/env python3
"""clip_bench.py - what a clip box (include/ovr_hip.h: ovr_hip_set_clip_box) costs and saves on the MI355X.

Legs:
  parent  `python bench.py --gpus 1 --steps K --warmup W --no-extras --no-views --no-skip-leg --no-cpu-baseline` of THIS tree and of `--parent-tree DIR`
          (a built checkout of the parent commit), alternated `--blocks` times each in child processes: the headline frame without a clip box.  The bar is
          the parent's own run-to-run spread - without a clip box this tree launches the kernels the parent launches (tools/kernel_metadata.py).
  cuts    the headline configuration (bench.py c3) in one process, one renderer, the states ALTERNATED in blocks of `--frames` frames so that all see the
          same machine state: no clip box; the volume cut in half ALONG the view (the half nearer to the camera along the view's dominant axis removed:
          every ray is shortened); the volume cut in half ACROSS the view (a cutting plane that contains the dominant axis: half the silhouette).  Per
          state: kernel / march / shade milliseconds, samples and shadow samples and their ratios against the unclipped frame, pipeline and layout.
One JSON line per leg on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lighting_bench import leg_parent, make_renderer, spread  # noqa: E402  (the same legs' plumbing)

INF = float("inf")


def cut_boxes(cam, n):
    """(name, lower, upper) of the two half cuts for a camera (eye, at, up) on an n^3 volume of spacing 1 at the origin"""
    view = [a - e for e, a in zip(cam[0], cam[1])]
    k = max(range(3), key=lambda i: abs(view[i]))                # the view's dominant axis
    j = min((i for i in range(3) if i != k), key=lambda i: abs(view[i]))   # the axis the view runs least along
    lo, hi = [-INF] * 3, [INF] * 3
    if view[k] > 0:
        lo[k] = n / 2.0                                           # the camera looks towards +k: the lower half is the near one
    else:
        hi[k] = n / 2.0
    along = ("half_along_view", tuple(lo), tuple(hi))
    lo, hi = [-INF] * 3, [INF] * 3
    hi[j] = n / 2.0
    return [along, ("half_across_view", tuple(lo), tuple(hi))]


def leg_cuts(ctx, args):
    ovr, torch, np, bench = ctx
    ren, cam = make_renderer(ovr, torch, np, bench)
    n = bench.CONFIGS["c3"]["n"]
    states = [("unclipped", None, None)] + cut_boxes(cam, n)
    res = {name: [] for name, _, _ in states}
    info = {}
    for _ in range(args.blocks):
        for name, lo, hi in states:
            if lo is None:
                ren.set_clip_box(None)
            else:
                ren.set_clip_box(lo, hi)
            ren.commit()
            for _ in range(args.settle):       # the tuner measures again after a box change, frame 1 sizes the request pool
                ren.render()
            k = m = s = 0.0
            for _ in range(args.frames):
                ren.render()
                st = ren.stats()
                k += st.kernel_ms; m += st.march_ms; s += st.shade_ms
            res[name].append((k / args.frames, m / args.frames, s / args.frames))
            info[name] = dict(pipeline=int(st.pipeline), layout=int(st.layout), tuning=int(st.tuning), samples=int(st.samples), shaded_samples=int(st.shaded_samples),
                              shadow_samples=int(st.shadow_samples), box=None if lo is None else [list(map(str, lo)), list(map(str, hi))])
    out = dict(leg="cuts", config="c3", frames_per_block=args.frames, blocks=args.blocks)
    base = info["unclipped"]
    for name, v in res.items():
        out[name] = dict(kernel_ms=spread([r[0] for r in v]), march_ms=spread([r[1] for r in v]), shade_ms=spread([r[2] for r in v]), **info[name],
                         samples_ratio=round(info[name]["samples"] / max(base["samples"], 1), 4),
                         shadow_samples_ratio=round(info[name]["shadow_samples"] / max(base["shadow_samples"], 1), 4))
    ren.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("legs", nargs="*", default=["cuts"], choices=["parent", "cuts"])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=60, help="frames per timed block")
    ap.add_argument("--settle", type=int, default=20, help="untimed frames after every box change")
    ap.add_argument("--blocks", type=int, default=3, help="how often every state (or tree) is measured, alternated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    ctx = None
    for leg in args.legs:
        if leg == "parent":
            rec = leg_parent(args)   # child processes only: nothing here has touched the GPU yet when this leg comes first
        else:
            if ctx is None:
                import numpy as np
                import torch
                import bench
                import ovr_amd as ovr
                if not torch.cuda.is_available():
                    raise SystemExit("clip_bench.py needs an MI355X")
                ctx = (ovr, torch, np, bench)
            rec = leg_cuts(ctx, args)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
