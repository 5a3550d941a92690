#!/usr/bin/env python3
"""projection_bench.py - what the projections (include/ovr_hip.h: ovr_hip_set_projection) cost on the MI355X.

Configurations: bench.py's c3 shape (1024^3 f32, 1920 x 1080: the headline volume and view) and c2 shape (512^3 f32, 1024 x 1024).  Per configuration, states
measured in ONE process and ALTERNATED in blocks of `--frames` frames, `--blocks` times each, so that all see the same machine state:

  baseline    the unshaded march (OVR_HIP_SHADE_NONE) under an ALL-ZERO alpha table, skipping off, the general layout forced: it walks the same rays, the same
              steps and the same voxels as a projection (no ray ends early).  `--parent-tree DIR` (a built checkout of the parent commit) measures the same
              state there, in a child process, before anything else: the baseline "on the parent commit".
  maximum     ovr_hip_set_projection(MAXIMUM), skipping off
  mean        ovr_hip_set_projection(MEAN)
  maximum+rs  MAXIMUM with range skipping (ovr_hip_set_empty_space_skipping(1)): the fraction of steps skipped and the time against `maximum`

on the bench's synthetic volume, and - `front` - on a volume with a bright structure in front of it (the synthetic field with a bright slab at the near face).
The tool ASSERTS that baseline samples == maximum samples == mean samples == maximum+rs samples + skipped_samples.
Reported per state: the median over the blocks of the per-block mean kernel_ms (device events around the frame's kernels), the spread between the blocks
(min, max), and the baseline's own block-to-block spread, beyond which alone a difference means anything.  Warm-up: `--settle` untimed frames per state.
One JSON line per configuration and volume on stdout; `--out FILE` also writes them there.

`--profile-state NAME` (baseline, maximum, mean, maximum+rs): no timing - ONE renderer in that state on the first configuration renders `--settle` + `--frames`
frames and the process ends: the program a counter collection runs (tools/projection_prof.sh: rocprofv3 --pmc, one counter set per run, no tracing)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"c3": dict(n=1024, width=1920, height=1080), "c2": dict(n=512, width=1024, height=1024)}

# the baseline state alone, for a tree that may not know the projections: run with cwd = the tree, prints one JSON line
BASELINE_CHILD = r'''
import json, sys
sys.path.insert(0, ".")
import numpy as np, torch
import ovr_amd as ovr
n, w, h, settle, frames, blocks = (int(x) for x in sys.argv[1:7])
dev = torch.device("cuda", 0)
vol = ovr.synth.make_volume_torch(n, dev, "float32")
colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
alphas = np.array(alphas, np.float32); alphas[1::2] = 0.0
cam = ovr.synth.make_camera("oblique", n)
ren = ovr.create_renderer("hip", 0)
ren.set_fbsize((w, h)); ren.set_frame_accumulation(True); ren.set_shading(0); ren.set_layout_choice(0); ren.set_empty_space_skipping(False)
ren.set_transfer_function(colors, alphas, vr)
ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
ren.set_camera(*cam); ren.set_sparse_sampling(False); ren.commit()
for _ in range(settle): ren.render()
rows = []
for _ in range(blocks):
    k = 0.0
    for _ in range(frames):
        ren.render(); k += ren.stats().kernel_ms
    rows.append(k / frames)
st = ren.stats()
print(json.dumps(dict(kernel_ms=rows, samples=int(st.samples), rays=int(st.rays), layout=int(st.layout))))
'''


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def parent_baseline(args, shape):
    if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "open-volume-renderer_amd")):
        return None
    env = dict(os.environ)
    env.pop("OVR_HIP_LIBRARY", None)
    out = subprocess.run([sys.executable, "-c", BASELINE_CHILD] + [str(shape[k]) for k in ("n", "width", "height")] + [str(args.settle), str(args.frames), str(args.blocks)],
                         cwd=args.parent_tree, env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        return dict(error=(out.stdout + out.stderr)[-600:])
    rec = json.loads(lines[-1])
    return dict(kernel_ms=spread(rec["kernel_ms"]), samples=rec["samples"], rays=rec["rays"], layout=rec["layout"])


def make_volume(ctx, n, front):
    ovr, torch, np = ctx
    vol = ovr.synth.make_volume_torch(n, torch.device("cuda", 0), "float32")
    if front:   # the oblique camera looks from -x, +y, +z: a bright slab at the low-x face lies in front of everything else
        vol[:, :, 2:2 + max(n // 32, 2)] = 0.97
    return vol


def make_renderer(ctx, shape, vol, projection, skipping):
    ovr, torch, np = ctx
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    if projection == 0:
        alphas = np.array(alphas, np.float32)
        alphas[1::2] = 0.0
    cam = ovr.synth.make_camera("oblique", shape["n"])
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((shape["width"], shape["height"]))
    ren.set_frame_accumulation(True)
    ren.set_shading(0)
    ren.set_layout_choice(0)
    ren.set_empty_space_skipping(skipping)
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam)
    ren.set_sparse_sampling(False)
    if projection:
        ren.set_projection(projection)
    ren.commit()
    return ren


def leg(ctx, args, name, front):
    ovr, torch, np = ctx
    shape = SHAPES[name]
    rec = dict(config=name, volume="front" if front else "synthetic", frames_per_block=args.frames, blocks=args.blocks, settle=args.settle)
    if not front:
        pb = parent_baseline(args, shape)   # a child process, before this process holds the volume
        if pb is not None:
            rec["parent_baseline"] = pb
    vol = make_volume(ctx, shape["n"], front)
    states = [("baseline", 0, False), ("maximum", ovr.PROJECT_MAXIMUM, False), ("mean", ovr.PROJECT_MEAN, False), ("maximum+rs", ovr.PROJECT_MAXIMUM, True)]
    rens = {s[0]: make_renderer(ctx, shape, vol, s[1], s[2]) for s in states}
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
    steps = int(st["baseline"].samples)
    assert st["baseline"].layout == 0 and st["baseline"].skipped_samples == 0
    assert int(st["maximum"].samples) == steps and int(st["mean"].samples) == steps, (steps, int(st["maximum"].samples), int(st["mean"].samples))
    assert int(st["maximum+rs"].samples + st["maximum+rs"].skipped_samples) == steps and rens["maximum+rs"].get_projection().range_skipping == 1
    if "parent_baseline" in rec and "samples" in rec["parent_baseline"]:
        assert rec["parent_baseline"]["samples"] == steps, (rec["parent_baseline"]["samples"], steps)
    rec["steps"] = steps
    rec["rays"] = int(st["baseline"].rays)
    for k in rens:
        rec[k] = dict(kernel_ms=spread(rows[k]))
    base = rec["baseline"]["kernel_ms"]
    rec["baseline_spread_ms"] = round(base["max"] - base["min"], 4)
    for k in ("maximum", "mean", "maximum+rs"):
        rec[k]["vs_baseline_ms"] = round(rec[k]["kernel_ms"]["median"] - base["median"], 4)
    rec["maximum+rs"]["skipped_fraction"] = round(int(st["maximum+rs"].skipped_samples) / max(steps, 1), 4)
    rec["maximum+rs"]["vs_maximum_ms"] = round(rec["maximum+rs"]["kernel_ms"]["median"] - rec["maximum"]["kernel_ms"]["median"], 4)
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
    ap.add_argument("--no-front", action="store_true", help="the synthetic volume alone")
    ap.add_argument("--profile-state", default=None, choices=["baseline", "maximum", "mean", "maximum+rs"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("projection_bench.py needs an MI355X")
    ctx = (ovr, torch, np)
    if args.profile_state:
        modes = {"baseline": (0, False), "maximum": (ovr.PROJECT_MAXIMUM, False), "mean": (ovr.PROJECT_MEAN, False), "maximum+rs": (ovr.PROJECT_MAXIMUM, True)}
        shape = SHAPES[args.configs[0]]
        ren = make_renderer(ctx, shape, make_volume(ctx, shape["n"], False), *modes[args.profile_state])
        for _ in range(args.settle + args.frames):
            ren.render()
        st = ren.stats()
        print(json.dumps(dict(profile_state=args.profile_state, config=args.configs[0], frames=args.settle + args.frames, samples=int(st.samples), skipped_samples=int(st.skipped_samples),
                              kernel_ms=round(st.kernel_ms, 4))), flush=True)
        ren.close()
        return
    lines = []
    for name in args.configs:
        for front in ((False,) if args.no_front else (False, True)):
            lines.append(json.dumps(leg(ctx, args, name, front)))
            print(lines[-1], flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
