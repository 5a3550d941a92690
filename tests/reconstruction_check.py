"""Child process of tests/test_reconstruction_gpu.py.

  exact              run with OVR_HIP_LIBRARY = libovr_hip_parity.so (the kernels built with -DOVR_PARITY_EXACT=1) and the oracle in its "det" mode: every marched
                     pixel then equals the oracle's bit for bit, so the chain  frame == model(A / N, G / N, N)  ends at the oracle: A is the ORACLE's accumulation
                     buffer, N the count of the oracle's sample lists, G the sum over those lists of the gradient pixels a run with the mode OFF shows
  overflow <out.npz> any library: an accumulating FILL run on the pooled pipeline whose frames, N, A and G are written to out.npz (the parent runs it with and
                     without OVR_HIP_POOL_CHUNKS=8, which makes an early frame overflow the request pool and be rendered twice, and compares)
Prints one line per part and "reconstruction_check: all exact"; exit code 1 on any difference."""
import ctypes as C
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, _R + "/tests", _R + "/oracle"]
import numpy as np  # noqa: E402
import ovr_amd as ovr  # noqa: E402
import oracle as O  # noqa: E402
from helpers import make_case, oracle_scene, hip_setup, hip_frame  # noqa: E402

M = ovr.reconstruction
f32 = np.float32
FOCUS = ((0.5, 0.5), 0.06, 0.07)   # the benchmark's


def bits_differ(a, b):
    return int((np.ascontiguousarray(a, f32).view(np.uint32) != np.ascontiguousarray(b, f32).view(np.uint32)).sum())


def noise_tile():
    return (np.random.default_rng(11).integers(0, 256, size=(32, 32, 64)) / 255.0).astype(f32)


def sparse_renderer(case, noise, pipeline, accumulate, mode=1):
    ren = ovr.create_renderer("hip")
    ren.set_layout_choice(0)
    hip_setup(ovr, ren, case, accumulate=accumulate, pipeline=pipeline)
    ren.set_noise_tile(noise)
    ren.set_focus(*FOCUS)
    ren.set_sparse_sampling(True)
    ren.set_reconstruction(mode)
    ren.commit()
    return ren


def exact():
    bad = 0
    noise = noise_tile()
    case = make_case(ovr, O, n=32, tf="bumps", cam="oblique", size=(100, 76), shading=2, spp=1)
    w, h = case["size"]
    sc = oracle_scene(O, case, sparse=True, focus=FOCUS, noise=noise)
    ren, off = sparse_renderer(case, noise, 2, True), sparse_renderer(case, noise, 2, True, mode=0)
    accum, rgba, grad = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), np.zeros((h, w, 3), f32)
    N, G = np.zeros((h, w), f32), np.zeros((h, w, 3), f32)
    for k in range(1, 7):
        cnt = O.Counters()
        sc.lib.ovr_oracle_render_frame(C.byref(sc.s), k, 1, O._fp(accum), O._fp(rgba), O._fp(grad), C.byref(cnt), 0)
        xy = O.sparse_mask(k, w, h, FOCUS[0], FOCUS[1], FOCUS[2], noise).reshape(-1, 2)
        N[xy[:, 1], xy[:, 0]] += f32(1)
        off.render()
        off_grad = hip_frame(ovr, off)[1]
        G[xy[:, 1], xy[:, 0]] = (G[xy[:, 1], xy[:, 0]] + off_grad[xy[:, 1], xy[:, 0]]).astype(f32)
        ren.render()
        got_rgba, got_grad = hip_frame(ovr, ren)
        d = [bits_differ(ren.reconstruction_weights(), N), bits_differ(ren.accumulation(0), accum), bits_differ(ren.reconstruction_gradient(), G)]
        exp_rgba, exp_grad = M.reconstruct(*M.level0(accum, G, N), N)
        d += [bits_differ(got_rgba, exp_rgba), bits_differ(got_grad, exp_grad)]
        print(f"exact: frame {k}: differing floats N {d[0]}, A {d[1]}, G {d[2]}, frame RGBA {d[3]}, gradient {d[4]}; sampled {int((N > 0).sum())} of {w * h}")
        bad += sum(d)
    ren.close()
    off.close()
    return bad


def overflow(path):
    noise = noise_tile()
    case = make_case(ovr, O, n=32, tf="bumps", cam="oblique", size=(100, 76), shading=2, spp=1)
    ren = sparse_renderer(case, noise, 2, True)
    out = {}
    for k in range(1, 7):
        ren.render()
        rgba, grad = hip_frame(ovr, ren)
        out[f"rgba{k}"], out[f"grad{k}"] = rgba, grad
        out[f"N{k}"], out[f"A{k}"], out[f"G{k}"] = ren.reconstruction_weights(), ren.accumulation(0), ren.reconstruction_gradient()
        out[f"chunks{k}"] = np.array([ren.stats().pool_chunks], np.int64)
    ren.close()
    np.savez(path, **out)
    print(f"overflow: wrote {len(out)} arrays")
    return 0


if __name__ == "__main__":
    part = sys.argv[1]
    n_bad = exact() if part == "exact" else overflow(sys.argv[2])
    if n_bad:
        print(f"reconstruction_check: {n_bad} floats differ")
        sys.exit(1)
    print("reconstruction_check: all exact")
