#!/usr/bin/env python3
"""preintegration_bench.py - what pre-integrated classification (include/ovr_hip.h: ovr_hip_set_preintegration) costs and buys on the MI355X.

The scene is tools/slice_context_bench.py's: the 1024^3 f32 synthetic volume at 1920 x 1080 under the oblique camera.

Timing run.  ONE renderer is switched between the states below in blocks of `--frames` frames, `--blocks` times each, ALTERNATED, so that all see the same machine
state; after every switch `--settle` untimed frames.  The general layout is forced and empty-space skipping is off in every state (the pre-integrated frame has
neither choice).  States:

  march@1           the unshaded march (OVR_HIP_SHADE_NONE) at sampling rate 1
  march@2           the same at rate 2 (the bar section 24 names: a pre-integrated rate-1 frame dearer than this is said so at its top)
  march@4           the same at rate 4, the shipped scene files' rate
  preintegrated@1   the pre-integrated frame at rate 1

Reported per state: the median over the blocks of the per-block mean kernel_ms (device events around the frame's kernels) with the blocks' min and max, and the
samples.

Quality run.  The same renderer under a thin-shell table (256 entries, zero but for two peaks three and four entries wide), one frame per state without
accumulation: the mean absolute RGBA difference of march@1, march@4 and preintegrated@1 from that renderer's march at rate 16, over the pixels any of the
four frames covers - and, beside it, the same over the premultiplied frames (rgb * a, a) and over alpha alone: the frames are un-premultiplied, so the colour
of a barely covered pixel weighs as much in the first figure as an opaque one's.

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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("preintegration_bench.py needs an MI355X")
    n = args.n
    OFF, SEGMENTS = ovr.preintegration.OFF, ovr.preintegration.SEGMENTS
    # state -> (pre-integration mode, sampling rate)
    states = {"march@1": (OFF, 1.0), "march@2": (OFF, 2.0), "march@4": (OFF, 4.0), "preintegrated@1": (SEGMENTS, 1.0)}
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

    def switch(mode, rate):
        ren.set_preintegration(mode)
        ren.set_volume_sampling_rate(rate)
        ren.commit()

    rows = {k: [] for k in states}
    stats = {}
    for _ in range(args.blocks):
        for name, (mode, rate) in states.items():
            switch(mode, rate)
            for _ in range(args.settle):
                ren.render()
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[name].append(t / args.frames)
            st = ren.stats()
            stats[name] = dict(samples=int(st.samples), shaded_samples=int(st.shaded_samples), rays=int(st.rays))
    g = ren.get_preintegration()
    rec = dict(n=n, width=args.width, height=args.height, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, timing=dict(table_entries=1024, nodes=int(g.nodes),
               subdivision=int(g.subdivision), states={}))
    for name in states:
        rec["timing"]["states"][name] = dict(kernel_ms=spread(rows[name]), samples=stats[name]["samples"], shaded_samples=stats[name]["shaded_samples"])
    med = {k: rec["timing"]["states"][k]["kernel_ms"]["median"] for k in states}
    rec["timing"]["preintegrated_vs_march1"] = round(med["preintegrated@1"] / med["march@1"], 4)
    rec["timing"]["preintegrated_vs_march2"] = round(med["preintegrated@1"] / med["march@2"], 4)
    rec["timing"]["preintegrated_vs_march4"] = round(med["preintegrated@1"] / med["march@4"], 4)

    # ---- quality: a thin-shell table, one frame per state, against the rate-16 march
    m = 256
    shell_colors, shell_alphas, _ = ovr.synth.make_tfn("dense", m, np.float32)
    shell_alphas = np.array(shell_alphas, np.float32).copy()
    a = np.zeros(m, np.float32)
    a[80:83] = 0.85
    a[164:168] = 0.6
    shell_alphas[1::2] = a
    ren.set_frame_accumulation(False)
    ren.set_transfer_function(shell_colors, shell_alphas, vr)

    def frame(mode, rate):
        switch(mode, rate)
        ren.render()
        fb = ovr.FrameBufferData()
        ren.mapframe(fb)
        return np.array(fb.rgba.data(), copy=True).astype(np.float64), ren.stats()

    truth, _ = frame(OFF, 16.0)
    frames = {name: frame(*states[name]) for name in ("march@1", "march@4", "preintegrated@1")}
    g = ren.get_preintegration()
    covered = truth[..., 3] > 0
    for f, _ in frames.values():
        covered |= f[..., 3] > 0
    quality = dict(table_entries=m, nodes=int(g.nodes), subdivision=int(g.subdivision), covered_pixels=int(covered.sum()), states={})
    def premultiplied(f):      # (the frames are un-premultiplied: the colour of a pixel of alpha 1e-6 weighs as much as an opaque one's)
        return np.concatenate([f[..., :3] * f[..., 3:], f[..., 3:]], -1)

    for name, (f, st) in frames.items():
        quality["states"][name] = dict(mean_abs_rgba_difference=round(float(np.abs(f - truth)[covered].mean()), 6), max_abs_rgba_difference=round(float(np.abs(f - truth)[covered].max()), 6),
                                       mean_abs_premultiplied_difference=round(float(np.abs(premultiplied(f) - premultiplied(truth))[covered].mean()), 6),
                                       mean_abs_alpha_difference=round(float(np.abs(f[..., 3] - truth[..., 3])[covered].mean()), 6),
                                       kernel_ms=round(float(st.kernel_ms), 4), samples=int(st.samples))
    rec["quality"] = quality
    ren.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
