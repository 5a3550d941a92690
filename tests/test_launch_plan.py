"""Which march / shade kernel variant a frame takes and what its launches need (csrc/host/launch_plan.hpp: addressing mode, row loads, LDS-staged
bricks, deep rounds, material and clipped variants, shade order, shade grid, LDS bytes) on the CPU: the header is free of HIP, so the host compiler
builds launch_plan_driver.cpp against it and every scenario of the driver is one test.  Every variant renders the same frame bit for bit, so a wrong
choice is invisible to the frame tests; the driver's tables are the launcher's rules as literals, and its sweep holds every plan to the predicates
the kernels' static_asserts use."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENARIOS = ["addressing", "row_loads", "inplace_unshaded", "inplace_shaded", "pooled", "deep_rounds", "shade_grid", "errors", "sweep"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("launch_plan") / "driver"
    # (no ROCm include path: the plan must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "launch_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_plan(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
