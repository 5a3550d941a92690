"""The host side of pre-integrated classification (csrc/host/preintegration_host.hpp) through a stand-alone program, built plainly and once more with the address
and undefined-behaviour sanitizers: its node table against the numpy model's (open-volume-renderer_amd/preintegration.py node_table) for the three transfer
functions of the tests and for tables of unequal lengths, the subdivision the LDS budget allows with its refusal, and OVR_HIP_PREINTEGRATION as data.  Both
sides sum in float64 and round once to float32, so a component differs by one float32 ulp at the most - at a rounding boundary, where log2 of the two maths
libraries may differ in its last bit.  No GPU, no ROCm headers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import preintegration_cases as QC
import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
F = np.float32
SCENARIOS = ["subdivision", "env_parser"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("preintegration_host_" + request.param) / "driver"
    # (no ROCm include path: the header must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], "-I", HOST, os.path.join(ROOT, "tests", "preintegration_host_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_scenario(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def _tables(ovr):
    out = {}
    for tf in QC.TFS:
        colors, alphas, _ = QC.transfer_function(ovr, tf, np.float32)
        out[tf] = PC.tables(colors, alphas)
    rng = np.random.default_rng(24)
    out["7 colours, 33 alphas"] = (rng.random((7, 3)).astype(F), rng.random(33).astype(F))
    out["40 colours, 5 alphas"] = (rng.random((40, 3)).astype(F), np.array([0.0, 1.0, 0.25, 1.5, -0.5], F))      # entries at, above and below the clamp
    out["one entry each"] = (np.array([[0.2, 0.4, 0.6]], F), np.array([0.3], F))
    return out


def _ulps(a, b):
    """the distance of two non-negative float32 arrays in units of the last place"""
    return np.abs(np.asarray(a, F).view(np.int32).astype(np.int64) - np.asarray(b, F).view(np.int32).astype(np.int64))


def test_node_table_vs_model(ovr, driver, tmp_path):
    P = ovr.preintegration
    for name, (ct, at) in _tables(ovr).items():
        for s in P.SUBDIVISIONS:
            path = tmp_path / "tables.bin"
            rgba = np.concatenate([ct, np.ones((len(ct), 1), F)], 1).astype(F)
            path.write_bytes(struct.pack("<3i", len(ct), len(at), s) + rgba.tobytes() + at.astype(F).tobytes())
            lines = subprocess.check_output([driver, "nodes", str(path)], text=True).split()
            m = int(lines[0])
            want = P.node_table(ct, at, s)
            assert m == len(want) == P.node_count(len(ct), len(at), s) and len(lines) == 1 + 4 * (m + 1), (name, s, m)
            got = np.array([int(x, 16) for x in lines[1:]], np.uint32).view(F).reshape(m + 1, 4)
            assert np.array_equal(got[m].view(np.uint32), got[m - 1].view(np.uint32)), (name, s, "the copy of the last node")
            d = _ulps(got[:m], want)
            print(name, s, "nodes", m, "differing components", int((d > 0).sum()), "max ulps", int(d.max()))
            assert d.max() <= 1, (name, s, int(d.max()))
            assert (d > 0).sum() <= 0.02 * d.size, (name, s, int((d > 0).sum()))     # only at a rounding boundary


def test_the_budget_is_stated_once_and_the_plugin_uses_the_parser(ovr):
    plan = open(os.path.join(HOST, "launch_plan.hpp")).read()
    assert plan.count("constexpr size_t kPreintegrationLdsBudget") == 1 and "three workgroups" in plan
    assert ovr.preintegration.LDS_BUDGET == (160 * 1024 // 3) // 16 * 16
    src = open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
    assert "preintegration_host.hpp" in src and "parse_preintegration(" in src and "OVR_HIP_PREINTEGRATION expects" in src and "ovr_hip_set_preintegration(h" in src
    assert "preintegration_host.hpp" in open(os.path.join(ROOT, "plugin", "Makefile")).read()
    assert "OVR_HIP_PREINTEGRATION" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
