#!/usr/bin/env python3
"""isosurface_context_bench.py - what the isosurface context (include/ovr_hip.h: ovr_hip_set_isosurface_context) costs on the MI355X.

The scene is tools/slice_context_bench.py's: the n^3 f32 synthetic volume under the oblique camera and the sparse transfer function, sampling rate 1 (the defaults:
1024^3 at 1920 x 1080; `--n 512 --width 1024 --height 1024` is the second shape).  ONE renderer is switched between the states below in blocks of `--frames`
frames, `--blocks` times each, ALTERNATED, so that all see the same machine state; after every switch `--settle` untimed frames.  States:

  march                the unshaded march (OVR_HIP_SHADE_NONE), skipping off, the general layout forced
  context/unreachable  the context frame with isovalues no sample reaches: the same steps through the new kernel
  opaque/<s>           the opaque 2-level isosurface frame under shading mode <s> (none, gradient, full), range skipping off
  layers/<s>           the translucent 2-level frame (opacities 0.4, 0.6)
  opaque+ctx/<s>, layers+ctx/<s>, opaque+ctx0.3/<s>, layers+ctx0.3/<s>   their context twins at scale 1 and 0.3
  opaque+ctx0/<s>, layers+ctx0/<s>   the twins at scale 0: the isosurface frame's events and shadow walks, bit for bit, through the fused kernel, which fetches and
                       classifies every step - the fusion's own cost on the isosurface side (`scale0_vs_frame`)
`--states a,b,...` restricts the run to the named states (counter runs).

The tool ASSERTS that `context/unreachable` has the counters of `march`.  Reported per state: the median over the blocks of the per-block mean kernel_ms (device
events around the frame's kernels) with the blocks' min and max, and the counters; `context/unreachable` against `march` of the same run beside the march's own
block-to-block spread, and every twin against march + its isosurface frame of the same run.  One JSON line on stdout; `--out FILE` also writes it there."""
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
    ap.add_argument("--frames", type=int, default=20, help="frames per timed block")
    ap.add_argument("--settle", type=int, default=3, help="untimed frames after every switch of state")
    ap.add_argument("--blocks", type=int, default=5, help="how often every state is measured, alternated")
    ap.add_argument("--states", default=None, help="comma-separated subset of the states")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("isosurface_context_bench.py needs an MI355X")
    n = args.n
    OFF, VOLUME = ovr.isosurface_context.OFF, ovr.isosurface_context.VOLUME
    levels, shells, unreachable = [0.5, 0.7], [0.4, 0.6], [50.0, 70.0]
    # state -> (shading, isovalues, opacities, context mode, opacity scale)
    states = {"march": (0, [], None, OFF, 1.0), "context/unreachable": (0, unreachable, None, VOLUME, 1.0)}
    for shading, tag in ((0, "none"), (1, "gradient"), (2, "full")):
        for name, op in (("opaque", None), ("layers", shells)):
            states[f"{name}/{tag}"] = (shading, levels, op, OFF, 1.0)
            states[f"{name}+ctx/{tag}"] = (shading, levels, op, VOLUME, 1.0)
            states[f"{name}+ctx0.3/{tag}"] = (shading, levels, op, VOLUME, 0.3)
            states[f"{name}+ctx0/{tag}"] = (shading, levels, op, VOLUME, 0.0)
    if args.states:
        states = {k: states[k] for k in args.states.split(",")}
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
        for name, (shading, iso, op, mode, scale) in states.items():
            ren.set_shading(shading)
            ren.set_isosurfaces(iso, op)
            ren.set_isosurface_context(mode, scale)
            ren.commit()
            for _ in range(args.settle):
                ren.render()
            t = 0.0
            for _ in range(args.frames):
                ren.render()
                t += ren.stats().kernel_ms
            rows[name].append(t / args.frames)
            st = ren.stats()
            stats[name] = dict(samples=int(st.samples), shaded_samples=int(st.shaded_samples), shadow_samples=int(st.shadow_samples), rays=int(st.rays))
    if "march" in states and "context/unreachable" in states:
        assert stats["context/unreachable"] == stats["march"], (stats["context/unreachable"], stats["march"])
    rec = dict(n=n, width=args.width, height=args.height, frames_per_block=args.frames, blocks=args.blocks, settle=args.settle, states={})
    for name in states:
        rec["states"][name] = dict(kernel_ms=spread(rows[name]), **{k: stats[name][k] for k in ("samples", "shaded_samples", "shadow_samples")})
    med = lambda k: rec["states"][k]["kernel_ms"]["median"]   # noqa: E731
    if "march" in states and "context/unreachable" in states:
        m = rec["states"]["march"]["kernel_ms"]
        rec["march_spread_ms"] = round(m["max"] - m["min"], 4)
        rec["unreachable_vs_march_ms"] = round(med("context/unreachable") - med("march"), 4)
        rec["unreachable_vs_march_ratio"] = round(med("context/unreachable") / med("march"), 4)
    rec["twins_vs_march_plus_frame"], rec["scale0_vs_frame"] = {}, {}
    for name in states:
        base = name.split("+")[0] + "/" + name.split("/")[-1]
        if "+ctx0/" in name and base in states:
            assert stats[name]["shaded_samples"] == stats[base]["shaded_samples"], (name, stats[name], stats[base])     # the same events
            rec["scale0_vs_frame"][name] = round(med(name) / med(base), 4)
        elif "+ctx" in name and base in states and "march" in states:
            rec["twins_vs_march_plus_frame"][name] = round(med(name) / (med("march") + med(base)), 4)
    ren.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
