"""The table of the known-answer ray queries (csrc/host/ray_query.hpp) and the frame kind (csrc/host/launch_plan.hpp frame_kind, committed_frame) on the CPU:
every entry's refusals - code, message and the order they are reported in - and its record size against literals, and frame_kind over the grid of facts the plan
drivers sweep, with the precedence cases written out by hand.  The driver (tests/ray_query_driver.cpp) holds the tables; no GPU, no ROCm headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENARIOS = ["preconditions", "arguments", "records", "precedence_table", "grid"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("ray_query") / "driver"
    # (no ROCm include path: the table and the plan must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "ray_query_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_scenario(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
