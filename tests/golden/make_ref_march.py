"""Generates tests/golden/ref_march.npz: what the reference's OWN ray-marching shader text computes on the scenes of ref_march_scenes.py.

oracle/_ref/ref_march_probe and ref_march_probe_fma (oracle/ref_march_probe.cpp, built by oracle/build_ref.sh) are the reference's
shaders_raymarching.cu + shaders_common.h compiled for the host, without and with contraction of a * b + c - the freedom nvcc has and
the reference does not fix.  The fixture keeps, per scene, the inputs (all but the volume, which ref_march_scenes.make_volume rebuilds
exactly; its CRC is kept), both builds' rgba and grad as float32 bit patterns, both builds' iteration counters and the camera basis as the reference's host
math (gdt, device_impl.cpp:125-144) hands it to the shader in the launch parameters (from the build without contraction).

Condition on the scene list, checked here: both builds give EQUAL counters on every scene.  A scene on which the reference disagrees
with itself about a count is replaced in ref_march_scenes.py (and the replacement noted there); this script refuses to write otherwise.

Run where the reference tree is present (after oracle/build_ref.sh):   python tests/golden/make_ref_march.py [--report]
--report additionally prints D (the largest difference between the two builds per quantity) and how far the frames move when the
texture filter's weights are rounded to 8 fractional bits as CUDA hardware keeps them; nothing of that goes into the fixture."""
import io
import json
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ref_march_scenes as RS  # noqa: E402

BUILDS = ("ref_march_probe", "ref_march_probe_fma")


def write_scene_file(path, scene, inp, fraction_bits=0):
    eye, at, up = inp["cam"]
    w, h = scene["size"]
    head = struct.pack("<5i6f2i2f9ff3if4i", 0x4D52564F, RS.REF_VALUE_TYPE[scene["dtype"]], *scene["dims"], *scene["origin"], *scene["spacing"],
                       inp["colors"].size // 3, inp["alphas"].size // 2, *scene["vr"], *eye, *at, *up, scene["fovy"], w, h, scene["spp"], scene["rate"],
                       scene["frames"], int(scene["accumulate"]), len(inp["pixels"]), fraction_bits)
    with open(path, "wb") as f:
        f.write(head)
        f.write(np.ascontiguousarray(inp["vol"]).tobytes())
        f.write(inp["colors"].astype("<f4").tobytes())
        f.write(inp["alphas"].astype("<f4").tobytes())
        f.write(inp["pixels"].astype("<i4").tobytes())


def run_probe(build, scene, inp, tmp, fraction_bits=0):
    """-> (rgba bits (h, w, 4) uint32, grad bits (h, w, 3) uint32, counters (2,) uint64, the launch parameters' camera (12,) float32)"""
    exe = os.path.join(ROOT, "oracle", "_ref", build)
    sf, of = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
    write_scene_file(sf, scene, inp, fraction_bits)
    subprocess.check_call([exe, sf, of])
    w, h = scene["size"]
    raw = np.fromfile(of, dtype=np.uint8)
    n = w * h
    assert raw.size == n * 28 + 16 + 48, (raw.size, n)
    rgba = raw[: n * 16].view("<u4").reshape(h, w, 4).copy()
    grad = raw[n * 16: n * 28].view("<u4").reshape(h, w, 3).copy()
    return rgba, grad, raw[n * 28: n * 28 + 16].view("<u8").copy(), raw[n * 28 + 16:].view("<f4").copy()


def probes_present():
    return all(os.path.exists(os.path.join(ROOT, "oracle", "_ref", b)) for b in BUILDS)


def generate():
    out, meta = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for i, scene in enumerate(RS.SCENES):
            inp = RS.build_inputs(scene)
            m = {k: (list(v) if isinstance(v, tuple) else v) for k, v in scene.items()}
            m["crc"] = inp["crc"]
            meta.append(m)
            out[f"s{i:02d}_colors"], out[f"s{i:02d}_alphas"] = inp["colors"], inp["alphas"]
            out[f"s{i:02d}_cam"] = np.concatenate(inp["cam"]).astype(np.float32)
            out[f"s{i:02d}_pixels"] = inp["pixels"]
            cnt = []
            for tag, build in zip(("", "_fma"), BUILDS):
                rgba, grad, c, basis = run_probe(build, scene, inp, tmp)
                out[f"s{i:02d}_rgba{tag}"], out[f"s{i:02d}_grad{tag}"] = rgba, grad
                cnt.append(c)
                if not tag:
                    out[f"s{i:02d}_basis"] = basis
            out[f"s{i:02d}_counters"] = np.stack(cnt)
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return out, meta


def save_deterministic(path, arrays):
    """an .npz np.load reads, with fixed member timestamps so that the same arrays always give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def quantities(rgba_bits, grad_bits):
    return RS.quantities(rgba_bits.view(np.float32), grad_bits.view(np.float32))


def report(out, meta):
    d = {"alpha": (0.0, ""), "colour": (0.0, ""), "grad": (0.0, "")}
    hw = {"alpha": (0.0, ""), "colour": (0.0, ""), "grad": (0.0, "")}
    hw8 = (0, "")
    with tempfile.TemporaryDirectory() as tmp:
        for i, scene in enumerate(RS.SCENES):
            qa, qb = quantities(out[f"s{i:02d}_rgba"], out[f"s{i:02d}_grad"]), quantities(out[f"s{i:02d}_rgba_fma"], out[f"s{i:02d}_grad_fma"])
            for k in d:
                v = float(np.abs(qa[k] - qb[k]).max())
                if v > d[k][0]:
                    d[k] = (v, scene["name"])
            rgba8, grad8, c8, _ = run_probe(BUILDS[0], scene, RS.build_inputs(scene), tmp, fraction_bits=8)
            q8 = quantities(rgba8, grad8)
            for k in hw:
                v = float(np.abs(qa[k] - q8[k]).max())
                if v > hw[k][0]:
                    hw[k] = (v, scene["name"])
            f = lambda bits: np.clip(np.nan_to_num(bits.view(np.float32)) * 255.0, 0, 255).astype(np.int32)   # truncation, as image_to_rgba8 does
            v = int(np.abs(f(out[f"s{i:02d}_rgba"]) - f(rgba8)).max())
            if v > hw8[0]:
                hw8 = (v, scene["name"])
    print("D = max |build_fma - build_nofma| over all scenes:")
    for k, (v, name) in d.items():
        print(f"  {k:7s} {v:.3e}   ({name})")
    print("filter weights rounded to 8 fractional bits vs exact weights (build without contraction):")
    for k, (v, name) in hw.items():
        print(f"  {k:7s} {v:.3e}   ({name})")
    print(f"  8-bit channels: {hw8[0]}   ({hw8[1]})")


def main():
    if not probes_present():
        sys.exit("oracle/_ref/ref_march_probe* not built: run oracle/build_ref.sh where the reference tree is present")
    out, meta = generate()
    bad = [m["name"] for i, m in enumerate(meta) if not (out[f"s{i:02d}_counters"][0] == out[f"s{i:02d}_counters"][1]).all()]
    for i, m in enumerate(meta):
        c = out[f"s{i:02d}_counters"]
        print(f"{i:2d} {m['name']:24s} primary {int(c[0, 0]):8d} shadow {int(c[0, 1]):9d}" + ("" if m["name"] not in bad else f"   != fma build {c[1].tolist()}"))
    if bad:
        sys.exit(f"the two builds of the reference disagree about a count on {bad}: replace these scenes in ref_march_scenes.py")
    path = os.path.join(HERE, "ref_march.npz")
    save_deterministic(path, out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(meta)} scenes")
    if "--report" in sys.argv[1:]:
        report(out, meta)


if __name__ == "__main__":
    main()
