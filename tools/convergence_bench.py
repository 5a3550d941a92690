#!/usr/bin/env python3
"""convergence_bench.py - what the convergence estimate and adaptive refinement (include/ovr_hip.h: ovr_hip_set_convergence) cost and save on the MI355X.

Legs (one process, one renderer per configuration; the modes are ALTERNATED in blocks inside the same run, so both see the same machine state):
  mode1   the headline configuration (bench.py c3: 1024^3 f32, 1920x1080, full shading, accumulation on): ms per frame with the mode OFF and with ESTIMATE,
          averaged over even and odd frames; `--blocks` pairs of blocks of `--frames` frames each
  idle    the same configuration, 1 sample per pixel, TEA jitter, ADAPTIVE with threshold 0: every frame is the same frame - ms per frame from frame 3 on
          (the resolve kernel and the host path) against the OFF frame
  c5      bench.py c5 (3840x2160, blue-noise jitter, 64 accumulated frames): frame error per even frame under ESTIMATE; then ADAPTIVE with the errors that run
          reported at frame 16 and at frame 64 as thresholds: active blocks per even frame and the time of the 64 frames against OFF's 64
  probe   (not in the default list) the fps `oracle/_ref/plugin_probe --loop` prints for the headline volume through the plugin, with and without OVR_HIP_CONVERGENCE=2

Every block is timed twice: by the host clock around its blocking render() calls and by two device events on the renderer's stream around them (the
renderer runs on a stream of this script's, ovr_hip_set_stream).  One JSON line per leg on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_renderer(ovr, torch, np, bench, name, stream, n_override=None, size_override=None):
    cfg = dict(bench.CONFIGS[name])
    n = n_override or cfg["n"]
    W, H = size_override or (cfg["width"], cfg["height"])
    dev = torch.device("cuda", 0)
    vol = ovr.synth.make_volume_torch(n, dev, cfg["dtype"])
    colors, alphas, vr = ovr.synth.make_tfn(cfg["tf"], 1024, np.float32)
    cam = ovr.synth.make_camera(cfg["cam"], n)
    ren = ovr.create_renderer("hip", 0)
    ren.set_stream(stream.cuda_stream)
    ren.set_fbsize((W, H))
    ren.set_frame_accumulation(True)
    ren.set_sample_per_pixel(cfg["spp"])
    ren.set_volume_sampling_rate(cfg["rate"])
    ren.set_shading(cfg["shading"])
    ren.set_transfer_function(colors, alphas, vr)
    if cfg.get("jitter") == "blue":
        ren.set_noise_tile(ovr.synth.make_noise_tile(64))
        ren.set_pixel_jitter(ovr.JITTER_BLUE_NOISE)
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=cfg["rate"]), ovr.Camera(*cam))
    ren.set_camera(*cam)
    ren.set_sparse_sampling(False)
    ren.commit()
    del vol
    torch.cuda.empty_cache()
    return ren, (W, H)


def timed_block(torch, ren, stream, frames, per_frame=None):
    """`frames` blocking render() calls: (host ms per frame, device-event ms per frame, mean kernel_ms)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kms = 0.0
    stream.synchronize()
    e0.record(stream)
    t0 = time.perf_counter()
    for _ in range(frames):
        ren.render()
        kms += ren.stats().kernel_ms
        if per_frame is not None:
            per_frame(ren)
    t1 = time.perf_counter()
    e1.record(stream)
    stream.synchronize()
    return (t1 - t0) * 1e3 / frames, e0.elapsed_time(e1) / frames, kms / frames


def settle(ren, limit=64):
    """frames until the layout / pipeline tuner and the background replica builds are done (they belong to no timed block)"""
    n = 0
    while n < limit:
        ren.render()
        n += 1
        st = ren.stats()
        if st.tuning != 1 and st.replicas_building == 0 and n >= 4:
            break
    return n


def restart(ren, mode, threshold=0.0, warm=8):
    """a new accumulation under `mode`; `warm` untimed frames (frame 1 sizes the request pool, the first frames page the layout in)"""
    ren.set_convergence(mode, threshold)
    ren.commit()
    for _ in range(warm):
        ren.render()


def spread(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4), n=len(xs))


def leg_mode1(ctx, args):
    ovr, torch, np, bench, stream = ctx
    ren, size = make_renderer(ovr, torch, np, bench, args.config, stream, args.n, args.size)
    extra = settle(ren)
    res = {0: [], 1: []}
    for _ in range(args.blocks):
        for mode in (0, 1):
            restart(ren, mode)
            res[mode].append(timed_block(torch, ren, stream, args.frames))
    c = ren.convergence()
    out = dict(leg="mode1", config=args.config, size=size, frames_per_block=args.frames, block_pairs=args.blocks, settle_frames=extra,
               off=dict(host_ms=spread([r[0] for r in res[0]]), event_ms=spread([r[1] for r in res[0]]), kernel_ms=spread([r[2] for r in res[0]])),
               estimate=dict(host_ms=spread([r[0] for r in res[1]]), event_ms=spread([r[1] for r in res[1]]), kernel_ms=spread([r[2] for r in res[1]])),
               frame_error=float(c.error), error_frames=int(c.frames), blocks_estimated=int(c.blocks))
    out["estimate_over_off_event_median"] = round(out["estimate"]["event_ms"]["median"] / out["off"]["event_ms"]["median"], 4)
    ren.close()
    return out


def leg_idle(ctx, args):
    ovr, torch, np, bench, stream = ctx
    ren, size = make_renderer(ovr, torch, np, bench, args.config, stream, args.n, args.size)
    ren.set_sample_per_pixel(1)
    ren.set_pixel_jitter(ovr.JITTER_TEA)
    ren.commit()
    extra = settle(ren)
    res = {0: [], 2: []}
    for _ in range(args.blocks):
        for mode in (0, 2):
            restart(ren, mode, 0.0)   # (8 warm-up frames: under ADAPTIVE everything is retired after the second)
            res[mode].append(timed_block(torch, ren, stream, args.frames))
    c, st = ren.convergence(), ren.stats()
    out = dict(leg="idle", config=args.config, size=size, frames_per_block=args.frames, block_pairs=args.blocks, settle_frames=extra,
               off=dict(host_ms=spread([r[0] for r in res[0]]), event_ms=spread([r[1] for r in res[0]])),
               adaptive=dict(host_ms=spread([r[0] for r in res[2]]), event_ms=spread([r[1] for r in res[2]]), kernel_ms=spread([r[2] for r in res[2]])),
               retired_blocks=int(c.retired_blocks), work_blocks=int(c.blocks), samples_last_frame=int(st.samples))
    out["speedup_host_median"] = round(out["off"]["host_ms"]["median"] / out["adaptive"]["host_ms"]["median"], 2)
    ren.close()
    return out


def leg_c5(ctx, args):
    ovr, torch, np, bench, stream = ctx
    ren, size = make_renderer(ovr, torch, np, bench, "c5", stream, args.n, args.size)
    extra = settle(ren)
    N = args.c5_frames

    def run(mode, threshold):
        restart(ren, mode, threshold, warm=0)
        trace = []

        def per_frame(r):
            c = r.convergence()
            if c.valid and c.frames == r.stats().frame_index:
                trace.append((int(c.frames), float(c.error), int(c.active_blocks)))
        host, event, kms = timed_block(torch, ren, stream, N, per_frame)
        return dict(total_host_ms=round(host * N, 3), total_event_ms=round(event * N, 3), kernel_ms_mean=round(kms, 4), threshold=threshold), trace

    off = [run(0, 0.0)[0] for _ in range(2)]
    est, trace = run(1, 0.0)
    err = {n: e for n, e, _ in trace}
    out = dict(leg="c5", size=size, frames=N, settle_frames=extra, off=off, estimate=est, blocks=int(ren.convergence().blocks),
               frame_error_by_frame={str(n): round(e, 6) for n, e in sorted(err.items())}, adaptive=[])
    for at in (16, N):
        if at not in err:
            continue
        r, tr = run(2, err[at])
        r["threshold_from_frame"] = at
        r["active_blocks_by_frame"] = {str(n): a for n, _, a in tr}
        r["final_error"] = tr[-1][1] if tr else None
        out["adaptive"].append(r)
    off2 = run(0, 0.0)[0]
    out["off"].append(off2)
    ren.close()
    return out


def leg_probe(ctx, args):
    """renderapp's loop (commit -> mapframe -> swap -> render, every frame mapped to the host) through the plugin: the fps oracle/_ref/plugin_probe --loop prints
    for the headline volume with and without OVR_HIP_CONVERGENCE=2, alternated"""
    import re
    import shutil
    import subprocess
    import tempfile
    ovr, torch, np, bench, stream = ctx
    probe, plugin = os.path.join(ROOT, "oracle", "_ref", "plugin_probe"), os.path.join(ROOT, "plugin", "libdevice_hip.so")
    if not (os.path.exists(probe) and os.path.exists(plugin)):
        return dict(leg="probe", skipped="oracle/_ref/plugin_probe or plugin/libdevice_hip.so missing")
    cfg = bench.CONFIGS[args.config]
    n = args.n or cfg["n"]
    W, H = args.size or (cfg["width"], cfg["height"])
    d = tempfile.mkdtemp(prefix="ovr_conv_", dir="/tmp")
    try:
        vol = ovr.synth.make_volume_torch(n, torch.device("cuda", 0), cfg["dtype"]).cpu().numpy()
        torch.cuda.empty_cache()
        _, alphas, _ = ovr.synth.make_tfn(cfg["tf"], 1024, np.float32)
        scene = ovr.vidi3d.write_scene(d, "c3", vol, ovr.synth._RAINBOW, alphas[1::2].copy(), (0.0, 1.0), ovr.synth.make_camera(cfg["cam"], n), fovy=45.0, sample_distance=1.0)
        del vol
        env = dict(os.environ, OVR_HIP_SKIP_EMPTY="0")
        env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.dirname(plugin), os.path.join(ROOT, "open-volume-renderer_amd"), env.get("LD_LIBRARY_PATH", "")])
        fps = {"off": [], "adaptive": []}
        last = ""
        for _ in range(2):
            for name, extra in (("off", {}), ("adaptive", {"OVR_HIP_CONVERGENCE": "2"})):
                out = subprocess.run([probe, "--loop", str(args.frames), scene, str(W), str(H)], env=dict(env, **extra), cwd=d, capture_output=True, text=True, timeout=600)
                m = re.search(r"loop fps = ([0-9.]+)", out.stdout)
                if out.returncode != 0 or not m:
                    return dict(leg="probe", error=(out.stdout + out.stderr)[-600:])
                fps[name].append(float(m.group(1)))
                if extra:
                    last = [l for l in out.stderr.splitlines() if "convergence:" in l][-1:]
        return dict(leg="probe", size=(W, H), volume=n, loop_frames=args.frames, fps_off=fps["off"], fps_adaptive=fps["adaptive"], device_line=last)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("legs", nargs="*", default=["mode1", "idle", "c5"], choices=["mode1", "idle", "c5", "probe"])
    ap.add_argument("--config", default="c3")
    ap.add_argument("--frames", type=int, default=200, help="frames per timed block")
    ap.add_argument("--blocks", type=int, default=3, help="alternated pairs of blocks")
    ap.add_argument("--c5-frames", type=int, default=64)
    ap.add_argument("--n", type=int, default=None, help="volume edge override (plumbing checks)")
    ap.add_argument("--size", type=lambda s: tuple(int(v) for v in s.split(",")), default=None, help="W,H override (plumbing checks)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import ovr_amd as ovr
    if not torch.cuda.is_available():
        raise SystemExit("convergence_bench.py needs an MI355X")
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    ctx = (ovr, torch, np, bench, stream)
    lines = []
    for leg in args.legs:
        rec = {"mode1": leg_mode1, "idle": leg_idle, "c5": leg_c5, "probe": leg_probe}[leg](ctx, args)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
