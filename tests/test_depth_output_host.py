"""The host side of the depth layer (csrc/host/depth_output_host.hpp) through a stand-alone program with its own main, built plainly and once more with the
address and undefined-behaviour sanitizers: what the setter accepts against the numpy model's check (open-volume-renderer_amd/depth_output.py), the activity
rule against the model's, and OVR_HIP_DEPTH_OUTPUT_FILE's encoder against the depth limit's reader (encode, then max_depth_decode: equal bits, +inf included)
and against numpy.  No GPU, no ROCm headers; nothing is loaded into Python under a sanitizer."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
F = np.float32
SCENARIOS = ["check", "activity", "resolve", "encoder"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("depth_output_host_" + request.param) / "driver"
    # (no ROCm include path: the header must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], "-I", HOST, os.path.join(ROOT, "tests", "depth_output_host_driver.cpp"), "-o", str(exe)])
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
    """the header accepts a mode and a threshold exactly where depth_output.check does"""
    D = ovr.depth_output
    thresholds = np.array([0.0, -0.0, np.finfo(F).tiny, 1e-45, 0.25, 0.5, 0.9, 0.9999, np.nextafter(F(0.9999), F(1)), 1.0, -0.5, np.inf, -np.inf, np.nan], F)
    refused = 0
    for mode, t in itertools.product((-1, 0, 1, 2), thresholds):
        got = int(subprocess.check_output([driver, "check", str(mode), _hex(t)], text=True))
        try:
            D.check(mode, t)
            want = True
        except ValueError:
            want = False
        assert (got == 0) == want, (mode, t, got)
        refused += got != 0
    assert 30 < refused < 4 * len(thresholds)


def test_the_activity_rule_vs_model(ovr):
    """the header's rule is stated once, and the model's table agrees with it (the driver's `activity` scenario holds the header to the same table)"""
    D = ovr.depth_output
    for mode, shading, slices, iso, proj, pre, gradop in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 2), (0, 3), (0, 1), (0, 1)):
        march = not slices and not iso and not proj
        preintegrated = march and shading == 0 and pre == 1
        gradient_opacity = gradop == 1 and march and shading in (0, 1) and not preintegrated
        want = mode == 1 and march and shading in (0, 1) and not preintegrated and not gradient_opacity
        assert D.active(mode, shading, slices, iso, proj, pre, gradop) == want, (mode, shading, slices, iso, proj, pre, gradop)
    hdr = open(os.path.join(HOST, "depth_output_host.hpp")).read()
    assert hdr.count("constexpr bool depth_output_active(") == 1 and "#include <hip" not in hdr
    frame = open(os.path.join(HOST, "frame.cpp")).read()
    plan = open(os.path.join(HOST, "launch_plan.hpp")).read()
    assert "depth_output_active(" in frame and "depth_output_active(" in plan and '#include "depth_output_host.hpp"' in plan
    assert "constexpr bool depth_output_active(" not in frame and "constexpr bool depth_output_active(" not in plan


def test_the_file_vs_numpy_and_the_models_resolve(ovr, driver, tmp_path):
    """the file OVR_HIP_DEPTH_OUTPUT_FILE names: depth_output.resolve's threshold depth of the layer, as numpy's little-endian float32 bytes - the format
    OVR_HIP_MAX_DEPTH reads"""
    rng = np.random.default_rng(27)
    w, h = 7, 5
    layer = np.zeros((h, w, 3), F)
    layer[..., 2] = rng.integers(0, 4, (h, w)).astype(F) / F(3)      # the share of three samples
    layer[..., 0] = np.where(layer[..., 2] > 0, (60.0 + 20.0 * rng.random((h, w))).astype(F) * layer[..., 2], 0).astype(F)
    layer[..., 1] = (30.0 * rng.random((h, w))).astype(F)
    assert (layer[..., 2] == 0).any() and (layer[..., 2] == 1).any()
    path = tmp_path / "depth.f32"
    out = subprocess.check_output([driver, "write", str(path), str(w), str(h)] + [_hex(v) for v in layer.reshape(-1)], text=True).strip()
    assert out == "written"
    got = np.fromfile(path, "<f4")
    want = ovr.depth_output.resolve(np.ones((h, w, 4), F), layer)[0]
    assert got.size == w * h and np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)) and np.isinf(got).any()
    assert ovr.max_depth.check(got, w, h).shape == (h, w)
    assert subprocess.check_output([driver, "write", str(tmp_path / "none" / "depth.f32"), "1", "1", _hex(1), _hex(1), _hex(1)], text=True).strip() == "refused"
    assert subprocess.check_output([driver, "write", str(path), "2", "1", _hex(1), _hex(1), _hex(1)], text=True).strip() == "refused"


def test_the_plugin_uses_the_encoder():
    src = open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
    assert "depth_output_host.hpp" in src and "depth_output_write_file(" in src and "ovr_hip_set_depth_output(h" in src
    assert 'getenv("OVR_HIP_DEPTH_OUTPUT")' in src and 'getenv("OVR_HIP_DEPTH_OUTPUT_FILE")' in src
    assert "depth_output_host.hpp" in open(os.path.join(ROOT, "plugin", "Makefile")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "OVR_HIP_DEPTH_OUTPUT" in text and "OVR_HIP_DEPTH_OUTPUT_FILE" in text
