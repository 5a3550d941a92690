#!/usr/bin/env python3
"""shadow_cache_bench.py - what the shadow cache (include/ovr_hip.h: ovr_hip_set_shadow_cache) costs and saves on the MI355X.

Legs:
  parent  `python bench.py --gpus 1 --steps K --warmup W --no-extras --no-views --no-skip-leg --no-cpu-baseline` of THIS tree and of `--parent-tree DIR`
          (a built checkout of the parent commit), alternated `--blocks` times each in child processes: the headline with the feature never enabled.  The
          expectation is no difference beyond the parent's own run-to-run spread - until the setter is called the frames run the kernels the parent runs.
  c3      the headline configuration (bench.py c3) at the sampling rates `--rates` (default 1 and 4: renderbatch's default and the scene files'): two
          renderers in one process, one marching its shadow rays, one reading the lattice, ALTERNATED in blocks of `--frames` frames so that both see the
          same machine state; per cell size of `--cells` (default 8, 4, 2): the build's milliseconds and iterations, the lattice's bytes, kernel / march /
          shade milliseconds of both, and the break-even frame count build_ms / (marched - cached).
  c4      the same for bench.py's c4, if it fits the sitting.
One JSON line per leg and rate on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARCHED, CACHED = 0, 1


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def leg_parent(args):
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "bench.py")):
        return dict(leg="parent", skipped="--parent-tree DIR: a built checkout of the parent commit")
    cmd = ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--no-extras", "--no-views", "--no-skip-leg", "--no-cpu-baseline"]
    res = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(args.blocks):
            for name, tree in (("parent", args.parent_tree), ("this", ROOT)):
                env = dict(os.environ)
                env.pop("OVR_HIP_LIBRARY", None)
                out = subprocess.run([sys.executable] + cmd + ["--detail-file", os.path.join(tmp, f"{name}.json")], cwd=tree, env=env, capture_output=True, text=True, timeout=900)
                lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
                if out.returncode != 0 or not lines:
                    return dict(leg="parent", error=(out.stdout + out.stderr)[-800:], tree=tree)
                res[name].append(json.loads(lines[-1]))
    out = dict(leg="parent", steps=args.steps, warmup=args.warmup, runs_each=args.blocks)
    for name, recs in res.items():
        for field in ("ms_per_step", "kernel_ms", "value"):
            if all(field in r for r in recs):
                out[f"{name}_{field}"] = spread([float(r[field]) for r in recs])
    return out


def make_renderer(ctx, config, rate):
    ovr, torch, np, bench = ctx
    cfg = dict(bench.CONFIGS[config])
    cfg["rate"] = rate
    dev = torch.device("cuda", 0)
    vol = ovr.synth.make_volume_torch(cfg["n"], dev, cfg["dtype"])
    colors, alphas, vr = ovr.synth.make_tfn(cfg["tf"], 1024, np.float32)
    cam = ovr.synth.make_camera(cfg["cam"], cfg["n"])
    ren = ovr.create_renderer("hip", 0)
    ren.set_fbsize((cfg["width"], cfg["height"]))
    ren.set_frame_accumulation(True)
    ren.set_sample_per_pixel(cfg["spp"])
    ren.set_volume_sampling_rate(cfg["rate"])
    ren.set_shading(cfg["shading"])
    ren.set_transfer_function(colors, alphas, vr)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=cfg["rate"]), ovr.Camera(*cam))
    ren.set_camera(*cam)
    ren.set_sparse_sampling(False)
    ren.commit()
    del vol
    torch.cuda.empty_cache()
    return ren


def timed(ren, frames):
    k = m = s = 0.0
    for _ in range(frames):
        ren.render()
        st = ren.stats()
        k += st.kernel_ms; m += st.march_ms; s += st.shade_ms
    return (k / frames, m / frames, s / frames), dict(pipeline=int(st.pipeline), layout=int(st.layout), tuning=int(st.tuning), shaded_samples=int(st.shaded_samples),
                                                      shadow_samples=int(st.shadow_samples))


def summary(rows, info):
    return dict(kernel_ms=spread([r[0] for r in rows]), march_ms=spread([r[1] for r in rows]), shade_ms=spread([r[2] for r in rows]), **info)


def leg_config(ctx, args, config):
    recs = []
    for rate in args.rates:
        marched, cached = make_renderer(ctx, config, rate), make_renderer(ctx, config, rate)
        frames = max(4, int(args.frames / max(1.0, rate)))
        for _ in range(args.settle):       # the tuner measures, frame 1 sizes the request pool
            marched.render()
        rec = dict(leg=config, rate=rate, frames_per_block=frames, blocks=args.blocks, cells={})
        for cell in args.cells:
            cached.set_shadow_cache(CACHED, cell)
            cached.commit()
            cached.render()                # builds the lattice in front of the frame
            sc = cached.shadow_cache()
            for _ in range(args.settle):
                cached.render()
            rows = {"marched": [], "cached": []}
            info = {}
            for _ in range(args.blocks):
                for name, ren in (("marched", marched), ("cached", cached)):
                    r, info[name] = timed(ren, frames)
                    rows[name].append(r)
            assert cached.shadow_cache().builds == sc.builds
            m, c = summary(rows["marched"], info["marched"]), summary(rows["cached"], info["cached"])
            gain = m["kernel_ms"]["median"] - c["kernel_ms"]["median"]
            rec["cells"][str(cell)] = dict(dims=list(sc.dims), lattice_bytes=int(sc.bytes), build_ms=round(sc.build_ms, 3), build_shadow_samples=int(sc.build_shadow_samples),
                                           marched=m, cached=c, break_even_frames=round(sc.build_ms / gain, 1) if gain > 0 else None)
        marched.close(); cached.close()
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("legs", nargs="*", default=["c3"], choices=["parent", "c3", "c4"])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40, help="frames per timed block at rate 1 (divided by the rate above it)")
    ap.add_argument("--settle", type=int, default=20, help="untimed frames after a change")
    ap.add_argument("--blocks", type=int, default=3, help="how often every state (or tree) is measured, alternated")
    ap.add_argument("--rates", type=lambda s: [float(x) for x in s.split(",")], default=[1.0, 4.0])
    ap.add_argument("--cells", type=lambda s: [int(x) for x in s.split(",")], default=[8, 4, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    ctx = None
    for leg in args.legs:
        if leg == "parent":
            recs = [leg_parent(args)]      # child processes only: nothing here has touched the GPU yet when this leg comes first
        else:
            if ctx is None:
                import numpy as np
                import torch
                import bench
                import ovr_amd as ovr
                if not torch.cuda.is_available():
                    raise SystemExit("shadow_cache_bench.py needs an MI355X")
                ctx = (ovr, torch, np, bench)
            recs = leg_config(ctx, args, leg)
        for rec in recs:
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
