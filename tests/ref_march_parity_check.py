"""Run by tests/test_ref_march_gpu.py in a child process with OVR_HIP_LIBRARY = libovr_hip_parity.so and OVR_ORACLE_POWF = det: the exact-parity build of the
kernels on every scene of tests/golden/ref_march.npz against the REFERENCE's frames - the same bar as the oracle's (tests/test_oracle_vs_ref_march.py): alpha,
premultiplied colour and premultiplied gradient within 4 x D of the nearer build of the reference, primary sample count equal to the reference's.  The kernels do not
shadow-march samples of opacity 0, the reference does: their shadow count must equal the oracle's count for the visible samples, and the oracle's count for all samples
the reference's.  Prints one line per scene and "all within the band" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import oracle as O  # noqa: E402
import ovr_amd as ovr  # noqa: E402
import ref_march_scenes as RS  # noqa: E402
from ref_march_common import FIXTURE, hip_render  # noqa: E402
from test_oracle_vs_ref_march import oracle_render  # noqa: E402


def main():
    assert ovr._lib.load().ovr_hip_built_for_exact_parity() == 1, "needs OVR_HIP_LIBRARY = libovr_hip_parity.so"
    O.set_powf_mode(O.POWF_DET)
    scenes, D = RS.load_fixture(FIXTURE)
    worst = {q: (0.0, "") for q in RS.QUANTITIES}
    bad = 0
    for s in scenes:
        ren = ovr.create_renderer("hip")
        rgba, grad, primary, shadow = hip_render(ovr, ren, s)
        ren.close()
        pixels = s["pixels"] if len(s["pixels"]) else None
        ex = RS.band_excess(s, D, rgba, grad, pixels=pixels)
        # the oracle with the same pow: shadow iterations of visible samples (what the kernels march) and of all samples (what the reference marches)
        sc_counts = oracle_counts(s)
        ok = all(r <= 1.0 for _, _, r in ex.values()) and primary == s["primary"] and shadow == sc_counts[1] and sc_counts[0] == s["shadow"]
        ok = ok and not (np.isnan(rgba).any() or np.isnan(grad).any())
        bad += not ok
        for q, (d, t, _) in ex.items():
            if d > worst[q][0]:
                worst[q] = (d, s["name"])
        print(f"{s['name']}: {'ok ' if ok else 'BAD'} primary {primary} / {s['primary']}, shadow {shadow} / oracle visible {sc_counts[1]}, oracle all {sc_counts[0]} / {s['shadow']}; "
              + ", ".join(f"{q} {d:.2e} / {t:.2e}" for q, (d, t, _) in ex.items()), flush=True)
    print("worst distance of the parity build from the nearer build of the reference: " + ", ".join(f"{q} {d:.2e} ({n})" for q, (d, n) in worst.items()))
    print("all within the band" if not bad else f"{bad} scenes outside the bar")
    return 1 if bad else 0


def oracle_counts(s):
    """(shadow iterations of all samples, of the samples with opacity > 0) over all frames, oracle in the mode set above"""
    import ctypes as C
    w, h = s["size"]
    sparse = len(s["pixels"]) > 0
    from ref_march_common import noise_tile_for
    sc = O.OracleScene(s["vol"], s["colors"], s["alphas"], s["vr"], s["cam"], w, h, fovy=s["fovy"], spp=s["spp"], rate=s["rate"], shading=O.SHADE_FULL,
                       grid_origin=s["origin"], grid_spacing=s["spacing"], sparse=sparse, noise=noise_tile_for(s) if sparse else None)
    rgba, grad, accum = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    tot = vis = 0
    for f in range(1, s["frames"] + 1):
        cnt = O.Counters()
        sc.lib.ovr_oracle_render_frame(C.byref(sc.s), f, int(bool(s["accumulate"])), fp(accum), fp(rgba), fp(grad), C.byref(cnt), 0)
        tot += cnt.shadow_samples
        vis += cnt.shadow_samples_visible
    return tot, vis


if __name__ == "__main__":
    sys.exit(main())
