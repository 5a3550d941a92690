#!/usr/bin/env python3
"""gradient_opacity_bench.py - what gradient opacity (include/ovr_hip.h: ovr_hip_set_gradient_opacity) costs on the MI355X.

The scene is tools/preintegration_bench.py's: the 1024^3 f32 synthetic volume at 1920 x 1080 under the oblique camera, sampling rate 1.

ONE renderer is switched between the states below in blocks of `--frames` frames, `--blocks` times each, ALTERNATED, so that all see the same machine state; after
every switch `--settle` untimed frames.  The general layout is forced and empty-space skipping is off in every state (the gradient-opacity frame has neither
choice).  The ramp's thresholds are the `--percentiles` (default 50 and 90) of gradient_opacity.magnitudes over a `--crop`^3 block from the middle of the volume.
States:

  OFF@NONE        the unshaded march
  RAMP@NONE       the gradient-opacity frame under shading NONE
  OFF@GRADIENT    the gradient-shaded march
  RAMP@GRADIENT   the gradient-opacity frame under shading GRADIENT

Reported per state: the median over the blocks of the per-block mean kernel_ms (device events around the frame's kernels) with the blocks' min and max, samples
and shaded_samples; and, for the RAMP states, the share of the steps that fetched a gradient, from ovr_hip_gradient_opacity_floats over every `--stride`-th
pixel's ray.

One JSON line on stdout; `--out FILE` also writes it there."""
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
    ap.add_argument("--crop", type=int, default=96, help="edge of the block the thresholds' percentiles are taken over")
    ap.add_argument("--percentiles", type=float, nargs=2, default=(50.0, 90.0))
    ap.add_argument("--stride", type=int, default=97, help="every stride-th pixel's ray goes through the known-answer entry")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("gradient_opacity_bench.py needs an MI355X")
    n = args.n
    G = ovr.gradient_opacity
    vol = ovr.synth.make_volume_torch(n, torch.device("cuda", 0), "float32")
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.float32)
    cam = ovr.synth.make_camera("oblique", n)
    c = min(args.crop, n)
    a = (n - c) // 2
    m = G.magnitudes(vol[a:a + c, a:a + c, a:a + c].cpu().numpy(), ovr.projection.normalized_range(vr, np.float32))
    lo, hi = (float(x) for x in np.percentile(m, args.percentiles))
    if not lo < hi:
        raise SystemExit(f"the percentiles {args.percentiles} of the crop's magnitudes do not give lo < hi: {lo}, {hi}")
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
    # state -> (gradient-opacity mode, shading mode)
    states = {"OFF@NONE": (G.OFF, 0), "RAMP@NONE": (G.RAMP, 0), "OFF@GRADIENT": (G.OFF, 1), "RAMP@GRADIENT": (G.RAMP, 1)}

    def switch(mode, shading):
        ren.set_gradient_opacity(mode, lo, hi)
        ren.set_shading(shading)
        ren.commit()

    rows = {k: [] for k in states}
    stats = {}
    for _ in range(args.blocks):
        for name, (mode, shading) in states.items():
            switch(mode, shading)
            assert ren.get_gradient_opacity().active == mode
            for _ in range(args.settle):
                ren.render()
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[name].append(t / args.frames)
            st = ren.stats()
            stats[name] = dict(samples=int(st.samples), shaded_samples=int(st.shaded_samples), rays=int(st.rays))
    # the share of the steps that fetched a gradient, over a subset of the frame's rays
    switch(G.RAMP, 0)
    cs = ren.get_camera()
    basis = tuple(np.array(list(v), np.float32) for v in (cs.pos, cs.dir, cs.hor, cs.ver))
    d = ovr.projection.pixel_rays(basis, args.width, args.height).reshape(-1, 3)[::max(args.stride, 1)]
    steps, gradients, _, shaded, _ = ren.gradient_opacity_rays(np.broadcast_to(basis[0], d.shape), d, 0)
    g = ren.get_gradient_opacity()
    rec = dict(n=n, width=args.width, height=args.height, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, crop=c, percentiles=list(args.percentiles),
               lo=float(g.lo), hi=float(g.hi), inv_ramp=float(g.inv_ramp), magnitudes=dict(median=round(float(np.median(m)), 6), max=round(float(m.max()), 6)),
               sampled_rays=dict(rays=int(len(d)), steps=int(steps.sum()), gradient_steps=int(gradients.sum()), opaque_steps=int(shaded.sum())), states={})
    for name in states:
        rec["states"][name] = dict(kernel_ms=spread(rows[name]), samples=stats[name]["samples"], shaded_samples=stats[name]["shaded_samples"])
    med = {k: rec["states"][k]["kernel_ms"]["median"] for k in states}
    rec["ramp_none_vs_off_none"] = round(med["RAMP@NONE"] / med["OFF@NONE"], 4)
    rec["ramp_none_vs_off_gradient"] = round(med["RAMP@NONE"] / med["OFF@GRADIENT"], 4)
    rec["ramp_gradient_vs_off_gradient"] = round(med["RAMP@GRADIENT"] / med["OFF@GRADIENT"], 4)
    ren.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
