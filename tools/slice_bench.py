#!/usr/bin/env python3
"""slice_bench.py - what the slice frames (include/ovr_hip.h: ovr_hip_set_slices) cost on the MI355X.

The scene is tools/projection_bench.py's c3 shape: the 1024^3 f32 synthetic volume at 1920 x 1080 under the oblique camera, sampling rate 1.  ONE renderer is
switched between the states below in blocks of `--frames` frames, `--blocks` times each, ALTERNATED, so that all see the same machine state; after every switch
`--settle` untimed frames.  States:

  march          the unshaded march (OVR_HIP_SHADE_NONE), skipping off, the general layout forced
  projection     ovr_hip_set_projection(MAXIMUM), skipping off
  axial          one plane z = n / 2                                       (the plane kernel)
  orthogonal     three planes x = y = z = n / 2
  oblique        one plane through the centre, normal (1, 2, -1)
  slab32         a 32-voxel MAXIMUM slab on the oblique plane               (the walk kernel)
  slab32+rs      the same with range skipping (ovr_hip_set_empty_space_skipping(1))
  mean32         the same slab, MEAN
  inf            the +inf MAXIMUM slab: the projection's work through the slice kernel

The tool ASSERTS that `inf` fetches what `projection` fetches and that slab32+rs's samples + skipped_samples are slab32's samples.  Reported per state: the median
over the blocks of the per-block mean kernel_ms (device events around the frame's kernels) with the blocks' min and max, the samples, and for `inf` the difference
to `projection` beside the projection's own block-to-block spread, beyond which alone a difference means anything.  One JSON line on stdout; `--out FILE` also
writes it there."""
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
        raise SystemExit("slice_bench.py needs an MI355X")
    n = args.n
    c = (n / 2.0,) * 3
    oblique = (1.0, 2.0, -1.0)
    inf = float("inf")
    MAX, MEAN = ovr.PROJECT_MAXIMUM, ovr.PROJECT_MEAN
    # state -> (projection, slices, range skipping)
    states = {
        "march": (0, None, False),
        "projection": (MAX, None, False),
        "axial": (0, [(c, (0, 0, 1))], False),
        "orthogonal": (0, [(c, (1, 0, 0)), (c, (0, 1, 0)), (c, (0, 0, 1))], False),
        "oblique": (0, [(c, oblique)], False),
        "slab32": (0, [(c, oblique, 32.0, MAX)], False),
        "slab32+rs": (0, [(c, oblique, 32.0, MAX)], True),
        "mean32": (0, [(c, oblique, 32.0, MEAN)], False),
        "inf": (0, [(c, oblique, inf, MAX)], False),
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
        for name, (projection, slices, skipping) in states.items():
            ren.set_projection(projection)
            ren.set_slices(slices)
            ren.set_empty_space_skipping(skipping)
            ren.commit()
            for _ in range(args.settle):
                ren.render()
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[name].append(t / args.frames)
            st = ren.stats()
            stats[name] = dict(samples=int(st.samples), skipped_samples=int(st.skipped_samples), rays=int(st.rays))
    assert stats["inf"]["samples"] == stats["projection"]["samples"], (stats["inf"], stats["projection"])
    assert stats["slab32+rs"]["samples"] + stats["slab32+rs"]["skipped_samples"] == stats["slab32"]["samples"], (stats["slab32+rs"], stats["slab32"])
    rec = dict(n=n, width=args.width, height=args.height, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, states={})
    for name in states:
        rec["states"][name] = dict(kernel_ms=spread(rows[name]), samples=stats[name]["samples"], skipped_samples=stats[name]["skipped_samples"])
    p = rec["states"]["projection"]["kernel_ms"]
    rec["projection_spread_ms"] = round(p["max"] - p["min"], 4)
    rec["inf_vs_projection_ms"] = round(rec["states"]["inf"]["kernel_ms"]["median"] - p["median"], 4)
    rec["slab32_skipped_fraction"] = round(stats["slab32+rs"]["skipped_samples"] / max(stats["slab32"]["samples"], 1), 4)
    ren.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
