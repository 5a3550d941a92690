#!/usr/bin/env python3
"""lighting_bench.py - what the light and material setters (include/ovr_hip.h: ovr_hip_set_light / ovr_hip_set_material) cost on the MI355X.

Legs:
  parent  `python bench.py --gpus 1 --steps K --warmup W --no-extras --no-views --no-skip-leg --no-cpu-baseline` of THIS tree and of `--parent-tree DIR`
          (a built checkout of the parent commit), alternated `--blocks` times each in child processes: the headline frame in the reference state.  The
          expectation is no difference beyond the parent's own run-to-run spread - the reference state runs the kernels the parent runs.
  states  the headline configuration (bench.py c3) in one process, one renderer, the states ALTERNATED in blocks of `--frames` frames so that all see the
          same machine state: the reference state, the interactive app's default material (0.6, 0.9, 0.4, 40), the light along +z, the light along the
          view direction.  Per state: kernel / march / shade milliseconds, shadow samples, which pipeline and layout ran.
  rate4   the same at sampling rate 4 (the shade kernel at vector issue 1.0): the reference state against the app's material, alternated.
(L2 hit rates need a counter run of their own: `tools/prof.sh` around `lighting_bench.py states --blocks 1`.)
One JSON line per leg on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
APP_MATERIAL = (0.6, 0.9, 0.4, 40.0)
REFERENCE = (0.5, 0.5, 0.0, 0.0)


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def leg_parent(args):
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "bench.py")):
        return dict(leg="parent", skipped="--parent-tree DIR: a built checkout of the parent commit")
    cmd = ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--no-extras", "--no-views", "--no-skip-leg", "--no-cpu-baseline"]
    res = {"parent": [], "this": []}
    keys = {}
    for _ in range(args.blocks):
        for name, tree in (("parent", args.parent_tree), ("this", ROOT)):
            env = dict(os.environ)
            env.pop("OVR_HIP_LIBRARY", None)
            out = subprocess.run([sys.executable] + cmd + ["--detail-file", os.path.join("/tmp", f"lighting_bench_{name}.json")], cwd=tree, env=env, capture_output=True, text=True,
                                 timeout=900)
            lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode != 0 or not lines:
                return dict(leg="parent", error=(out.stdout + out.stderr)[-800:], tree=tree)
            rec = json.loads(lines[-1])
            keys[name] = sorted(rec)[:40]
            res[name].append(rec)

    def pick(recs, *names):
        for n in names:
            if all(n in r for r in recs):
                return spread([float(r[n]) for r in recs]), n
        return None, None
    out = dict(leg="parent", steps=args.steps, warmup=args.warmup, runs_each=args.blocks)
    for name in res:
        for field in (("ms_per_step", "step_ms", "ms_per_frame"), ("kernel_ms", "kernel_ms_per_step"), ("value",)):
            s, n = pick(res[name], *field)
            if s:
                out[f"{name}_{n}"] = s
        out[f"{name}_first_record"] = {k: v for k, v in res[name][0].items() if isinstance(v, (int, float, str)) and len(str(v)) < 40}
    return out


def make_renderer(ovr, torch, np, bench, rate=None):
    cfg = dict(bench.CONFIGS["c3"])
    if rate:
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
    return ren, cam


def run_states(ren, states, frames, blocks, settle=20):
    """every state `blocks` times, alternated; a block = the state's commit, `settle` untimed frames (the tuner measures again after a light or material
    change, frame 1 sizes the request pool), then `frames` timed ones"""
    res = {name: [] for name, _, _ in states}
    info = {}
    for _ in range(blocks):
        for name, light, material in states:
            ren.set_light_direction(light[0], light[1])
            ren.set_material(*material)
            ren.commit()
            for _ in range(settle):
                ren.render()
            k = m = s = 0.0
            for _ in range(frames):
                ren.render()
                st = ren.stats()
                k += st.kernel_ms; m += st.march_ms; s += st.shade_ms
            res[name].append((k / frames, m / frames, s / frames))
            info[name] = dict(pipeline=int(st.pipeline), layout=int(st.layout), tuning=int(st.tuning), shaded_samples=int(st.shaded_samples), shadow_samples=int(st.shadow_samples))
    return {name: dict(kernel_ms=spread([r[0] for r in v]), march_ms=spread([r[1] for r in v]), shade_ms=spread([r[2] for r in v]), **info[name]) for name, v in res.items()}


def leg_states(ctx, args):
    ovr, torch, np, bench = ctx
    ren, cam = make_renderer(ovr, torch, np, bench)
    view = tuple(float(e - a) for e, a in zip(cam[0], cam[1]))   # from the volume towards the camera: the light behind the viewer
    states = [("reference", (None, 1.0), REFERENCE), ("app_material", (None, 1.0), APP_MATERIAL), ("light_+z", ((0.0, 0.0, 1.0), 1.0), REFERENCE),
              ("light_along_view", (view, 1.0), REFERENCE)]
    out = dict(leg="states", config="c3", frames_per_block=args.frames, blocks=args.blocks, **run_states(ren, states, args.frames, args.blocks))
    ren.close()
    return out


def leg_rate4(ctx, args):
    ovr, torch, np, bench = ctx
    ren, _ = make_renderer(ovr, torch, np, bench, rate=4.0)
    states = [("reference", (None, 1.0), REFERENCE), ("app_material", (None, 1.0), APP_MATERIAL)]
    frames = max(4, args.frames // 4)
    out = dict(leg="rate4", config="c3 at rate 4", frames_per_block=frames, blocks=args.blocks, **run_states(ren, states, frames, args.blocks, settle=16))
    ren.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("legs", nargs="*", default=["states", "rate4"], choices=["parent", "states", "rate4"])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=60, help="frames per timed block")
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
                    raise SystemExit("lighting_bench.py needs an MI355X")
                ctx = (ovr, torch, np, bench)
            rec = {"states": leg_states, "rate4": leg_rate4}[leg](ctx, args)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
