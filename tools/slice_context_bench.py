#!/usr/bin/env python3
"""slice_context_bench.py - what the slice context (include/ovr_hip.h: ovr_hip_set_slice_context) costs on the MI355X.

The scene is tools/slice_bench.py's: the 1024^3 f32 synthetic volume at 1920 x 1080 under the oblique camera, sampling rate 1.  ONE renderer is switched between
the states below in blocks of `--frames` frames, `--blocks` times each, ALTERNATED, so that all see the same machine state; after every switch `--settle`
untimed frames.  States:

  march           the unshaded march (OVR_HIP_SHADE_NONE), skipping off, the general layout forced
  context/unmet   the context frame whose slices no ray meets: the same steps through the new kernel
  plane           one oblique plane through the centre, normal (1, 2, -1)        (the plane kernel)
  plane+ctx       the same plane with the context in front, scale 1
  plane+ctx0.3    the same at scale 0.3
  slab32          a 32-voxel MAXIMUM slab on the oblique plane                    (the walk kernel)
  slab32+ctx      the same slab with the context in front, scale 1

The tool ASSERTS that `context/unmet` fetches and shades what `march` does.  Reported per state: the median over the blocks of the per-block mean kernel_ms (device
events around the frame's kernels) with the blocks' min and max, the samples and shaded samples, and for `context/unmet` the ratio to `march` beside the march's
own block-to-block spread, beyond which alone a difference means anything.  One JSON line on stdout; `--out FILE` also writes it there."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=30, help="frames per timed block")
    ap.add_argument("--settle", type=int, default=5, help="untimed frames after every switch of state")
    ap.add_argument("--blocks", type=int, default=5, help="how often every state is measured, alternated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("slice_context_bench.py needs an MI355X")
    n = args.n
    c = (n / 2.0,) * 3
    oblique = (1.0, 2.0, -1.0)
    MAX = ovr.PROJECT_MAXIMUM
    OFF, FRONT = ovr.slice_context.OFF, ovr.slice_context.FRONT
    unmet = [((-100.0 * n, 0.0, 0.0), (1.0, 0.0, 0.0))]      # a plane far outside the box, behind the camera
    # state -> (slices, context mode, opacity scale)
    states = {
        "march": (None, OFF, 1.0),
        "context/unmet": (unmet, FRONT, 1.0),
        "plane": ([(c, oblique)], OFF, 1.0),
        "plane+ctx": ([(c, oblique)], FRONT, 1.0),
        "plane+ctx0.3": ([(c, oblique)], FRONT, 0.3),
        "slab32": ([(c, oblique, 32.0, MAX)], OFF, 1.0),
        "slab32+ctx": ([(c, oblique, 32.0, MAX)], FRONT, 1.0),
    }
    vol = ovr.synth.make_volume_torch(n, torch.device("cuda", 0), "float32")
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((args.width, args.height))
    ren.set_frame_accumulation(True)
    ren.set_shading(0)
    ren.set_layout_choice(0)
    ren.set_empty_space_skipping(False)
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=1.0), ovr.Camera(*cam))
    ren.set_camera(*cam)
    ren.set_sparse_sampling(False)
    ren.commit()
    del vol
    torch.cuda.empty_cache()
    rows = {k: [] for k in states}
    stats = {}
    for _ in range(args.blocks):
        for name, (slices, mode, scale) in states.items():
            ren.set_slices(slices)
            ren.set_slice_context(mode, scale)
            ren.commit()
            for _ in range(args.settle):
                ren.render()
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[name].append(t / args.frames)
            st = ren.stats()
            stats[name] = dict(samples=int(st.samples), shaded_samples=int(st.shaded_samples), rays=int(st.rays))
    assert stats["context/unmet"] == stats["march"], (stats["context/unmet"], stats["march"])
    rec = dict(n=n, width=args.width, height=args.height, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, states={})
    for name in states:
        rec["states"][name] = dict(kernel_ms=spread(rows[name]), samples=stats[name]["samples"], shaded_samples=stats[name]["shaded_samples"])
    m = rec["states"]["march"]["kernel_ms"]
    u = rec["states"]["context/unmet"]["kernel_ms"]
    rec["march_spread_ms"] = round(m["max"] - m["min"], 4)
    rec["unmet_vs_march_ms"] = round(u["median"] - m["median"], 4)
    rec["unmet_vs_march_ratio"] = round(u["median"] / m["median"], 4)
    ren.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
