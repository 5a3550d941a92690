"""Child process of tests/test_convergence_gpu.py.

  buffers / adaptive / static   run with OVR_HIP_LIBRARY = libovr_hip_parity.so (the kernels built with -DOVR_PARITY_EXACT=1) and the oracle in its "det" mode, as
                                tests/parity_exact_check.py is: every frame then equals the oracle's bit for bit, so the accumulation buffers, the retirement frames and
                                the resolved pixels of the convergence estimate can be held to the numpy model (ovr_amd.convergence) fed with the ORACLE's frames
  overflow <out.npz>            any library: an adaptive run whose frames, block errors and retirement frames are written to out.npz (the parent runs it with and
                                without OVR_HIP_POOL_CHUNKS=8, which forces the request pool to overflow, and compares)
Prints one line per part and "convergence_exact_check: all exact"; exit code 1 on any difference."""
import ctypes as C
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, _R + "/tests", _R + "/oracle"]
import numpy as np  # noqa: E402
import ovr_amd as ovr  # noqa: E402
import oracle as O  # noqa: E402
from helpers import make_case, oracle_scene, hip_setup, hip_frame  # noqa: E402

M = ovr.convergence
f32 = np.float32
bad = 0


def bits_differ(a, b):
    return int((np.asarray(a, f32).view(np.uint32) != np.asarray(b, f32).view(np.uint32)).sum())


def oracle_single_frames(sc, frames):
    w, h = sc.s.width, sc.s.height
    out = []
    for k in range(1, frames + 1):
        rgba, grad = np.zeros((h, w, 4), f32), np.zeros((h, w, 3), f32)
        cnt = O.Counters()
        sc.lib.ovr_oracle_render_frame(C.byref(sc.s), k, 0, None, O._fp(rgba), O._fp(grad), C.byref(cnt), 0)
        out.append((rgba, grad))
    return out


def adaptive_case():
    return make_case(ovr, O, n=32, tf="dense", cam="oblique", size=(192, 128), shading=2, spp=2)


def adaptive_threshold(frames):
    s = M.accumulate(frames[:4])
    E = M.block_errors(s[3][1], s[3][2], 4)
    return f32(np.median(E[E > 0]))


def buffers():
    """A == the float32 running sum of the oracle's single frames, H == that of the even ones - also behind a camera change that moves the empty blocks"""
    global bad
    ren = ovr.create_renderer("hip")
    report = []
    for step, cam in enumerate(("front", "oblique")):
        case = make_case(ovr, O, n=32, tf="sparse", cam=cam, size=(100, 76), shading=2, spp=2)
        fr = [f[0] for f in oracle_single_frames(oracle_scene(O, case), 6)]
        sums = M.accumulate(fr)
        if step == 0:
            hip_setup(ovr, ren, case, accumulate=True)
            ren.set_convergence(1)
        else:
            ren.set_camera(*case["cam"])
        ren.commit()
        for n in range(1, 7):
            ren.render()
            if n < 2:
                continue
            dA, dH = bits_differ(ren.accumulation(0), sums[n - 1][1]), bits_differ(ren.accumulation(1), sums[n - 1][2])
            report.append((cam, n, dA, dH))
            bad += dA + dH
        assert (sums[5][2] == 0).all(axis=-1).mean() > 0.05   # (some of the image is empty: what H must read 0 in)
    ren.close()
    print(f"buffers: (camera, n, floats of A that differ, of H) {report}", flush=True)


def adaptive():
    """retirement frames == the model's simulation on the oracle's frames; the mapped frame == A_{n_b} / n_b per block, in both framebuffer sets"""
    global bad
    case = adaptive_case()
    N = 16
    single = oracle_single_frames(oracle_scene(O, case), N)
    fr = [f[0] for f in single]
    t = adaptive_threshold(fr)
    want_nb, want_E, want_img = M.retirement_frames(fr, t)
    _, _, want_img15 = M.retirement_frames(fr[:N - 1], t)
    hit = np.zeros(want_nb.shape, bool)   # blocks whose pixels are not all 0 in every frame (the others may or may not get a workgroup: E_b = 0 either way)
    total = M.accumulate(fr)[-1][1]
    for j in range(hit.shape[0]):
        for i in range(hit.shape[1]):
            hit[j, i] = bool((total[j * 8:j * 8 + 8, i * 8:i * 8 + 8] != 0).any())
    late, still = int(((want_nb > 2) & hit).sum()), int(((want_nb == 0) & hit).sum())
    nblk = want_nb.size
    print(f"adaptive: threshold {t:.6g}; model: {int((want_nb == 2).sum())} of {nblk} blocks retire at frame 2, {late} later, {still} still active after frame {N}", flush=True)
    if late < 0.05 * nblk or still < 0.05 * nblk:
        bad += 1
        print("adaptive: the case is vacuous", flush=True)
    for swap in (True, False):
        ren = ovr.create_renderer("hip")
        hip_setup(ovr, ren, case, accumulate=True)
        ren.set_convergence(2, float(t))
        ren.commit()
        for n in range(1, N + 1):
            ren.render()
            if swap and n < N:
                ren.swap()
        err, frames = ren.convergence_blocks()
        got_nb = np.where(frames < 0, -frames, 0)
        d_nb = int(((got_nb != want_nb) & hit).sum()) + int((~np.isin(got_nb[~hit], (0, 2))).sum())
        d_E = bits_differ(err[hit], want_E[hit])
        rgba, grad = hip_frame(ovr, ren)
        d_img = bits_differ(rgba, want_img)
        # the gradient layer of a retired block is that of frame n_b, of an active one that of the last frame
        want_grad = single[N - 1][1].copy()
        for j, i in zip(*np.nonzero(want_nb > 0)):
            want_grad[j * 8:j * 8 + 8, i * 8:i * 8 + 8] = single[want_nb[j, i] - 1][1][j * 8:j * 8 + 8, i * 8:i * 8 + 8]
        d_grad = bits_differ(grad, want_grad)
        d_other = 0
        if swap:   # the other set holds frame N - 1: the same rule one frame earlier
            ren.swap()
            d_other = bits_differ(hip_frame(ovr, ren)[0], want_img15)
        c = ren.convergence()
        ok_counts = c.retired_blocks == int((got_nb > 0).sum()) and c.blocks == c.active_blocks + c.retired_blocks and c.frames == N and c.valid == 1
        ren.close()
        print(f"adaptive (swap every frame: {swap}): blocks whose retirement frame differs {d_nb}, E_b bits {d_E}, mapped RGBA floats {d_img}, gradient floats {d_grad}, "
              f"other set {d_other}, counts consistent {ok_counts}", flush=True)
        bad += d_nb + d_E + d_img + d_grad + d_other + (0 if ok_counts else 1)


def static():
    """one sample per pixel, TEA: every frame is the same frame S - threshold 0 retires everything after frame 2 and frames 3 ... 10 are S, marching nothing"""
    global bad
    case = make_case(ovr, O, n=32, tf="sparse", cam="oblique", size=(100, 76), shading=2, spp=1)
    S, G = oracle_single_frames(oracle_scene(O, case), 1)[0]
    ren = ovr.create_renderer("hip")
    hip_setup(ovr, ren, case, accumulate=True)
    ren.set_convergence(2, 0.0)
    ren.commit()
    report = []
    for n in range(1, 11):
        ren.render()
        rgba, grad = hip_frame(ovr, ren)
        st, c = ren.stats(), ren.convergence()
        d = bits_differ(rgba, S) + bits_differ(grad, G)
        if n in (1, 2):   # (S + S) / 2 == S exactly
            ok = st.samples > 0 and c.active_blocks == (c.blocks if n == 1 else 0)
        else:
            ok = st.samples == 0 and c.active_blocks == 0 and c.retired_blocks == c.blocks > 0 and c.error == 0.0 and c.valid == 1 and c.frames == 2
        report.append((n, d, bool(ok)))
        bad += d + (0 if ok else 1)
        ren.swap()
    ren.close()
    print(f"static: (frame, floats that differ from the oracle's single frame, state ok) {report}", flush=True)


def overflow(path):
    """an adaptive run, pooled from frame 2 on; everything that must not depend on whether the request pool overflowed goes to `path`"""
    case = adaptive_case()
    fr = [f[0] for f in oracle_single_frames(oracle_scene(O, case), 4)]
    t = adaptive_threshold(fr)
    ren = ovr.create_renderer("hip")
    hip_setup(ovr, ren, case, accumulate=True, pipeline=1)
    ren.set_layout_choice(0)
    ren.set_convergence(2, float(t))
    ren.commit()
    out = {}
    for n in range(1, 9):
        if n == 2:   # from the second frame on through the request pool (no accumulation reset: both pipelines give the same frame) - the pool's first use
            ren.set_shading_pipeline(2)
            ren.commit()
        ren.render()
        if n == 2:
            assert ren.stats().pipeline == 2 and ren.stats().frame_index == 2
        rgba, grad = hip_frame(ovr, ren)
        err, frames = ren.convergence_blocks()
        st = ren.stats()
        out.update({f"rgba{n}": rgba, f"grad{n}": grad, f"err{n}": err, f"frames{n}": frames, f"rays{n}": np.int64(st.rays), f"samples{n}": np.int64(st.samples)})
        ren.swap()
    ren.close()
    np.savez(path, **out)
    print(f"overflow: wrote {path}", flush=True)


if __name__ == "__main__":
    parts = sys.argv[1:] or ["buffers", "adaptive", "static"]
    if parts[0] == "overflow":
        overflow(parts[1])
        sys.exit(0)
    assert ovr._lib.load().ovr_hip_built_for_exact_parity() == 1, "this check needs libovr_hip_parity.so (OVR_HIP_LIBRARY)"
    O.set_powf_mode(O.POWF_DET)
    for part in parts:
        {"buffers": buffers, "adaptive": adaptive, "static": static}[part]()
    print("convergence_exact_check:", "all exact" if bad == 0 else f"{bad} difference(s)", flush=True)
    sys.exit(1 if bad else 0)
