"""The host side of the depth limit (csrc/host/max_depth_host.hpp) through a stand-alone program, built plainly and once more with the address and
undefined-behaviour sanitizers: what the setter accepts against the numpy model's check (open-volume-renderer_amd/max_depth.py), the activity rule against the
model's, the cut against the model's bit for bit, and OVR_HIP_MAX_DEPTH - a raw little-endian float32 file - as data.  No GPU, no ROCm headers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
F = np.float32
SCENARIOS = ["check", "activity", "cut", "file_parser"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("max_depth_host_" + request.param) / "driver"
    # (no ROCm include path: the header must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], "-I", HOST, os.path.join(ROOT, "tests", "max_depth_host_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_scenario(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def _hex(x):
    return "%08x" % int(np.asarray(x, F).view(np.uint32))


def test_the_setters_check_vs_model(ovr, driver):
    """the header accepts a size exactly where max_depth.check does"""
    M = ovr.max_depth
    sizes = (-1, 0, 1, 2, 37, 46340, 46341, 65536, 2 ** 31 - 1)
    checked = refused = 0
    for w, h in itertools.product(sizes, sizes):
        got = int(subprocess.check_output([driver, "check", "0", str(w), str(h)], text=True))
        try:
            M.check(np.zeros(w * h if 0 < w * h <= 64 else 1, F), w, h)
            want = True
        except ValueError as e:
            want = "holds width * height values" in str(e)      # (the model also holds the array to the size; the size itself was accepted)
        assert (got == 0) == want, (w, h, got)
        checked += 1
        refused += got != 0
    assert checked == 81 and 30 < refused < checked
    assert int(subprocess.check_output([driver, "check", "2", "4", "4"], text=True)) != 0 and int(subprocess.check_output([driver, "check", "1", "4", "4"], text=True)) == 0


def test_the_cut_vs_model(ovr, driver):
    M = ovr.max_depth
    values = np.array([0.0, 1.5, 61.32, 78.0, 3.4028235e38, -2.0, np.inf, -np.inf, np.nan, 1e-30], F)      # (no -0: fmin(0, -0) may give either zero)
    for t1, z in itertools.product(values[:5], values):
        got = subprocess.check_output([driver, "cut", _hex(t1), _hex(z)], text=True).strip()
        want = M.cut(np.array([t1], F), np.array([z], F))[0]
        assert got == _hex(want), (t1, z, got, _hex(want))


def test_the_file_vs_numpy(driver, tmp_path):
    """the file OVR_HIP_MAX_DEPTH names: numpy's little-endian float32 bytes come back value for value; any other length is refused"""
    rng = np.random.default_rng(26)
    image = (60.0 + 20.0 * rng.random((23, 37))).astype("<f4")
    image[3, 5], image[4, 6], image[0, 0] = np.inf, np.nan, -1.0
    path = tmp_path / "depth.f32"
    image.tofile(path)
    got = subprocess.check_output([driver, "file", str(path), "37", "23"], text=True).split()
    assert got == [_hex(v) for v in image.reshape(-1)]      # pixel (ix, iy) at ix + iy * width
    for w, h in ((23, 37), (37, 23)):
        assert (subprocess.check_output([driver, "file", str(path), str(w), str(h)], text=True).strip() != "refused") == (w * h == image.size)
    for w, h in ((37, 22), (38, 23), (0, 23), (37, 0), (851, 0)):
        assert subprocess.check_output([driver, "file", str(path), str(w), str(h)], text=True).strip() == "refused", (w, h)
    with open(path, "ab") as f:
        f.write(b"\0")
    assert subprocess.check_output([driver, "file", str(path), "37", "23"], text=True).strip() == "refused"
    assert subprocess.check_output([driver, "file", str(tmp_path / "missing.f32"), "37", "23"], text=True).strip() == "refused"


def test_the_activity_rule_vs_model(ovr):
    """the header's rule is stated once, and the model's table agrees with it (the driver's `activity` scenario holds the header to the same table)"""
    M = ovr.max_depth
    for on, shading, slices, iso, proj, pre, gradop, same in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 2), (0, 3), (0, 1), (0, 1), (0, 1)):
        march = not slices and not iso and not proj
        preintegrated = march and shading == 0 and pre == 1
        gradient_opacity = gradop == 1 and march and shading in (0, 1) and not preintegrated
        want = on == 1 and march and shading in (0, 1) and not preintegrated and not gradient_opacity and same == 1
        got = M.active(on, (40, 28), (40, 28) if same else (40, 27), shading, slices, iso, proj, pre, gradop)
        assert got == want, (on, shading, slices, iso, proj, pre, gradop, same)
    hdr = open(os.path.join(HOST, "max_depth_host.hpp")).read()
    assert hdr.count("constexpr bool max_depth_active(") == 1 and "#include <hip" not in hdr
    frame = open(os.path.join(HOST, "frame.cpp")).read()
    assert "max_depth_active(" in frame
    assert "max_depth_active(" in open(os.path.join(HOST, "launch_plan.hpp")).read()


def test_the_plugin_uses_the_parser():
    src = open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
    assert "max_depth_host.hpp" in src and "max_depth_read_file(" in src and "OVR_HIP_MAX_DEPTH expects" in src and "ovr_hip_set_max_depth(h" in src
    assert "max_depth_host.hpp" in open(os.path.join(ROOT, "plugin", "Makefile")).read()
    assert "OVR_HIP_MAX_DEPTH" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
