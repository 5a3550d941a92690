#!/usr/bin/env python3
"""update_bench.py - what ovr_hip_update_volume (include/ovr_hip.h) costs against ovr_hip_set_volume on the MI355X.

Legs:
  parent  `python bench.py --gpus 1 ...` of THIS tree and of `--parent-tree DIR` (a built checkout of the parent commit), alternated `--blocks` times each
          in child processes: the headline frame, which no update touches (tools/lighting_bench.py's leg).
  update  on C3's volume (bench.py c3: 1024^3 f32) and on a 256^3 u8 volume, in one warm process per volume, with resident replicas (layouts mode 2) and
          without (mode 0), all from device memory:
            whole   the whole-volume update against set_volume, alternating, `--blocks` runs each: the whole call and its kernels' share
            box64   a 64^3 box (update only), `--blocks` runs            box256  a 256^3 box
            series  frames per second of a ten-step series (two arrays, alternating) played through update_volume and through set_volume, one frame per step
One JSON line per case on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lighting_bench import leg_parent, spread  # noqa: E402


def cases_for(ctx, args, name, n, dtype, size, layouts):
    ovr, torch, np, bench = ctx
    dev = torch.device("cuda", 0)
    vols = [ovr.synth.make_volume_torch(n, dev, dtype)]
    vols.append(vols[0].flip(0).contiguous())   # the series' other step: the same field, mirrored in z
    colors, alphas, vr = ovr.synth.make_tfn("sparse", 1024, np.dtype(dtype))
    cam = ovr.synth.make_camera("oblique", n)
    ren = ovr.create_renderer("hip", 0)
    ren.set_volume_layouts(layouts)
    ren.set_fbsize(size)
    ren.set_frame_accumulation(False)
    ren.set_shading(2)
    ren.set_transfer_function(colors, alphas, vr)
    scenes = [ovr.Scene(volume=v, transfer_function=None, volume_sampling_rate=1.0) for v in vols]
    ren.init(scenes[0], ovr.Camera(*cam))
    ren.commit()
    base = dict(leg="update", volume=name, n=n, dtype=dtype, layouts_mode=layouts, resident_gb=round(ren.volume_info().resident_bytes / 1e9, 3), runs=args.blocks)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for k in range(2):   # warm: the first set_volume of a process pays the fresh allocations, the first update nothing
        ren._upload_volume(scenes[k])
        ren.update_volume(vols[k], (0, 0, 0))
    res = dict(update_call=[], update_kernels=[], set_call=[], set_kernels=[])
    for k in range(args.blocks):
        res["update_call"].append(timed(lambda: ren.update_volume(vols[k % 2], (0, 0, 0))))
        res["update_kernels"].append(ren.update_times()["kernels_ms"])
        res["set_call"].append(timed(lambda: ren._upload_volume(scenes[k % 2])))
        res["set_kernels"].append(ren.upload_times()["kernels_ms"])
    yield dict(base, case="whole", **{f"{k}_ms": spread(v) for k, v in res.items()}, set_alloc_ms=round(ren.upload_times()["alloc_ms"], 4))
    whole_ms = sorted(res["update_call"])[len(res["update_call"]) // 2]
    for edge in (64, 256):
        if edge > n:
            continue
        box = vols[1][:edge, :edge, :edge].contiguous()
        lower = (min((n - edge) // 2 + 1, n - edge),) * 3   # unaligned on purpose where the box is smaller than the volume
        call, kern = [], []
        for _ in range(args.blocks + 1):
            call.append(timed(lambda: ren.update_volume(box, lower)))
            kern.append(ren.update_times()["kernels_ms"])
        med = sorted(call[1:])[len(call[1:]) // 2]
        yield dict(base, case=f"box{edge}", update_call_ms=spread(call[1:]), update_kernels_ms=spread(kern[1:]), ratio_to_whole=round(med / whole_ms, 5),
                   ratio_of_voxels=round((edge / n) ** 3, 7))
    fps = {}
    for how in ("update_volume", "set_volume"):
        def step(k):
            if how == "update_volume":
                ren.update_volume(vols[k % 2], (0, 0, 0))
            else:
                ren._upload_volume(scenes[k % 2])
            ren.render()
        step(0)
        ms = timed(lambda: [step(k) for k in range(1, 11)])
        fps[how] = round(10.0 / (ms * 1e-3), 2)
    yield dict(base, case="series", steps=10, fbsize=list(size), frames_per_second=fps)
    ren.close()
    del vols, scenes
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("legs", nargs="*", default=["update"], choices=["parent", "update"])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4, help="how often every case (or tree) is measured, alternated")
    ap.add_argument("--volumes", default="c3,u8_256", help="which volumes the update leg measures")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for leg in args.legs:
        if leg == "parent":
            emit(leg_parent(args))   # child processes only: nothing here has touched the GPU yet when this leg comes first
            continue
        import numpy as np
        import torch
        import bench
        import ovr_amd as ovr
        if not torch.cuda.is_available():
            raise SystemExit("update_bench.py needs an MI355X")
        ctx = (ovr, torch, np, bench)
        c3 = bench.CONFIGS["c3"]
        for name, n, dtype, size in (("c3", c3["n"], c3["dtype"], (c3["width"], c3["height"])), ("u8_256", 256, "uint8", (1024, 768))):
            if name not in args.volumes.split(","):
                continue
            for layouts in (0, 2):
                for rec in cases_for(ctx, args, name, n, dtype, size, layouts):
                    emit(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
