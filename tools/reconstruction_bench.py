#!/usr/bin/env python3
"""reconstruction_bench.py - what the pull-push reconstruction of sparse-sampled frames (include/ovr_hip.h: ovr_hip_set_reconstruction) costs on the MI355X.

The benchmark's foveated configuration (bench.py c3 --sparse-sampling: 1024^3 f32, 1920x1080, full shading, focus (0.5, 0.5), 0.06, 0.07) is rendered with
the mode OFF and FILL in ALTERNATING blocks of frames inside one process and one renderer, so both see the same machine state; once without and once with
accumulation.  Per mode: the host time per blocking render(), the device-event time per frame on the renderer's stream, the frame's own kernel_ms (which
the reconstruction is never part of) and reconstruct_ms (two events around the reconstruction's launches; phase timing is on).  Also: the launches FILL
adds per frame and the bytes per second its level-0 passes achieve against their compulsory traffic.
One JSON line per leg on stdout; `--out FILE` also writes them there."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FOCUS = ((0.5, 0.5), 0.06, 0.07)   # apps/main_app.cpp:123-124, bench.py --sparse-sampling


def make_renderer(ovr, torch, np, bench, stream, n, size, accumulate):
    cfg = dict(bench.CONFIGS["c3"])
    dev = torch.device("cuda", 0)
    vol = ovr.synth.make_volume_torch(n, dev, cfg["dtype"])
    colors, alphas, vr = ovr.synth.make_tfn(cfg["tf"], 1024, np.float32)
    cam = ovr.synth.make_camera(cfg["cam"], n)
    ren = ovr.create_renderer("hip", 0)
    ren.set_stream(stream.cuda_stream)
    ren.set_fbsize(size)
    ren.set_frame_accumulation(accumulate)
    ren.set_sample_per_pixel(cfg["spp"])
    ren.set_volume_sampling_rate(cfg["rate"])
    ren.set_shading(cfg["shading"])
    ren.set_transfer_function(colors, alphas, vr)
    ren.set_noise_tile(ovr.synth.make_noise_tile(64))
    ren.init(ovr.Scene(volume=vol, transfer_function=None, volume_sampling_rate=cfg["rate"]), ovr.Camera(*cam))
    ren.set_camera(*cam)
    ren.set_focus(*FOCUS)
    ren.set_sparse_sampling(True)
    ren.set_phase_timing(True)
    ren.commit()
    del vol
    torch.cuda.empty_cache()
    return ren


def launches_added(ovr, size, accumulate):
    """kernels and memsets FILL enqueues behind a frame: the list scatter, one pull pass per three levels down to the first level of at most 64 x 64 texels, the
    one-workgroup pass over the top of the pyramid, one push pass per finer level; without accumulation also the clear of N"""
    lv = ovr.reconstruction.levels(*size)
    top = next(i for i, (w, h) in enumerate(lv) if w <= 64 and h <= 64)
    return 1 + (top + 2) // 3 + 1 + top + (0 if accumulate else 1)


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


def timed_block(torch, ren, stream, frames):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kms = rms = 0.0
    stream.synchronize()
    e0.record(stream)
    t0 = time.perf_counter()
    for _ in range(frames):
        ren.render()
        kms += ren.stats().kernel_ms
        rms += ren.reconstruction().reconstruct_ms
    t1 = time.perf_counter()
    e1.record(stream)
    stream.synchronize()
    return (t1 - t0) * 1e3 / frames, e0.elapsed_time(e1) / frames, kms / frames, rms / frames


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024, help="volume edge (default: the benchmark's 1024)")
    ap.add_argument("--size", default="1920,1080")
    ap.add_argument("--frames", type=int, default=40, help="frames per block")
    ap.add_argument("--blocks", type=int, default=5, help="pairs of OFF / FILL blocks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import ovr_amd as ovr
    size = tuple(int(v) for v in args.size.split(","))
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    lines = []
    for accumulate in (False, True):
        ren = make_renderer(ovr, torch, np, bench, stream, args.n, size, accumulate)
        settled = settle(ren)
        rows = {0: [], 1: []}
        info = None
        for _ in range(args.blocks):
            for mode in (0, 1):
                ren.set_reconstruction(mode)
                ren.commit()
                for _ in range(3):   # (the mode's buffers, the pool's size: not in the timed block)
                    ren.render()
                rows[mode].append(timed_block(torch, ren, stream, args.frames))
                if mode == 1:
                    info = ren.reconstruction()
        med = {m: [statistics.median(r[i] for r in rows[m]) for i in range(4)] for m in (0, 1)}
        pixels = size[0] * size[1]
        # compulsory traffic of the level-0 passes: the pull reads RGBA + gradient + N (32 B per pixel; with accumulation A and G instead of the set, the same),
        # the push reads them again and writes RGBA + gradient of the holes (28 B); level 1 is written once and read once (2 x 32 B per four pixels)
        level0_bytes = pixels * (32 + 32 + 28 + 16)
        leg = dict(leg="accumulate" if accumulate else "single_frame", n=args.n, size=list(size), focus=[list(FOCUS[0]), FOCUS[1], FOCUS[2]], frames_per_block=args.frames,
                   blocks=args.blocks, settle_frames=settled,
                   off=dict(host_ms=med[0][0], device_ms=med[0][1], kernel_ms=med[0][2], reconstruct_ms=med[0][3]),
                   fill=dict(host_ms=med[1][0], device_ms=med[1][1], kernel_ms=med[1][2], reconstruct_ms=med[1][3]),
                   fill_over_off_device_ms=med[1][1] - med[0][1], fill_over_off_fraction=(med[1][1] - med[0][1]) / med[0][1] if med[0][1] > 0 else None,
                   blocks_off_device_ms=[r[1] for r in rows[0]], blocks_fill_device_ms=[r[1] for r in rows[1]],
                   levels=int(info.levels), sampled_pixels=int(info.sampled_pixels), filled_pixels=int(info.filled_pixels),
                   launches_added=launches_added(ovr, size, accumulate),
                   level0_bytes=level0_bytes, reconstruct_gb_per_s=(level0_bytes / (med[1][3] * 1e-3) / 1e9) if med[1][3] > 0 else None)
        line = json.dumps(leg)
        print(line, flush=True)
        lines.append(line)
        ren.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
