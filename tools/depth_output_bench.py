#!/usr/bin/env python3
"""depth_output_bench.py - what the depth layer (include/ovr_hip.h: ovr_hip_set_depth_output) costs on the MI355X.

The scene is tools/max_depth_bench.py's: the 1024^3 f32 synthetic volume at 1920 x 1080 under the oblique camera, sampling rate 1.

ONE renderer is switched between the states below in blocks of `--frames` frames, `--blocks` times each, ALTERNATED, so that all see the same machine state; after
every switch `--settle` untimed frames.  The general layout is forced and empty-space skipping is off in every state (the depth frame has neither choice).
States, each under shading NONE and GRADIENT:

  OFF      the march
  INF      the depth-limited frame under an image of +inf: the march's steps, drawn by the depth-limited kernel - the kernel that does the same work minus the
           depth accumulators
  DEPTH    the depth frame (threshold `--threshold`), no depth image: the march's steps, drawn by the new kernel
  BOTH     the depth frame with the +inf image committed: the new kernel with its depth load

Reported per state: the median over the blocks of the per-block mean kernel_ms (device events around the frame's kernels) with the blocks' min and max, samples
and shaded_samples; the ratios DEPTH / OFF, DEPTH / INF and BOTH / INF per shading mode.

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
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--frames", type=int, default=30, help="frames per timed block")
    ap.add_argument("--settle", type=int, default=5, help="untimed frames after every switch of state")
    ap.add_argument("--blocks", type=int, default=5, help="how often every state is measured, alternated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("depth_output_bench.py needs an MI355X")
    n = args.n
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
    inf = np.full((args.height, args.width), np.inf, np.float32)
    # (image, threshold) per state
    kinds = {"OFF": (None, None), "INF": (inf, None), "DEPTH": (None, args.threshold), "BOTH": (inf, args.threshold)}
    states = {f"{name}@{label}": (name, shading) for label, shading in (("NONE", 0), ("GRADIENT", 1)) for name in kinds}

    def switch(name, shading):
        image, tau = kinds[name]
        ren.set_max_depth(image)
        ren.set_depth_output(tau)
        ren.set_shading(shading)
        ren.commit()
        g = ren.get_depth_output()
        assert (g.active, g.limited) == (int(tau is not None), int(tau is not None and image is not None)), (name, g.active, g.limited)

    rows = {k: [] for k in states}
    stats = {}
    reached = {}
    for _ in range(args.blocks):
        for key, (name, shading) in states.items():
            switch(name, shading)
            for _ in range(args.settle):
                ren.render()
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[key].append(t / args.frames)
            st = ren.stats()
            stats[key] = dict(samples=int(st.samples), shaded_samples=int(st.shaded_samples), rays=int(st.rays))
            if name == "DEPTH" and key not in reached:      # what the layer holds, once
                fb = ovr.FrameBufferData()
                ren.mapframe(fb)
                layer = np.array(fb.grad.data(), copy=True).reshape(args.height, args.width, 3)
                rgba = np.array(fb.rgba.data(), copy=True).reshape(args.height, args.width, 4)
                thr, mean, share = ovr.depth_output.resolve(rgba, layer)
                hit = np.isfinite(thr)
                reached[key] = dict(pixels_reached=int(hit.sum()), threshold_depth=dict(min=round(float(thr[hit].min()), 3), max=round(float(thr[hit].max()), 3)) if hit.any() else None,
                                    pixels_lit=int(np.isfinite(mean).sum()))
    rec = dict(n=n, width=args.width, height=args.height, threshold=args.threshold, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, states={}, layer=reached)
    for key in states:
        rec["states"][key] = dict(kernel_ms=spread(rows[key]), samples=stats[key]["samples"], shaded_samples=stats[key]["shaded_samples"])
    med = {k: rec["states"][k]["kernel_ms"]["median"] for k in states}
    for label in ("NONE", "GRADIENT"):
        rec[f"depth_vs_off_{label.lower()}"] = round(med[f"DEPTH@{label}"] / med[f"OFF@{label}"], 4)
        rec[f"depth_vs_inf_{label.lower()}"] = round(med[f"DEPTH@{label}"] / med[f"INF@{label}"], 4)
        rec[f"both_vs_inf_{label.lower()}"] = round(med[f"BOTH@{label}"] / med[f"INF@{label}"], 4)
    ren.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
