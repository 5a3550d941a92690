"""The orthographic part of the launch plan (csrc/host/launch_plan.hpp: LaunchFacts::orthographic, LaunchPlan::orthographic, the variant predicates) on the
CPU, built and run the way tests/test_projection_plan.py does its driver: with orthographic == false every sampled plan is what it was; an orthographic frame
plans the clipped variants - the plan of the same frame with a clip box -, never LDS staging or deep rounds; the predicates the kernels' static_asserts ask
agree with the plan.  And OVR_HIP_ORTHOGRAPHIC as the plugin parses it (plugin/orthographic_env.hpp): a height > 0 or `auto`, the whole string consumed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "open-volume-renderer_amd", "csrc", "host")
SCENARIOS = ["off_changes_nothing", "orthographic_plans", "variants"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("camera_plan") / "driver"
    # (no ROCm include path: the plan must not need one)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HOST, os.path.join(ROOT, "tests", "camera_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_driver_runs_every_scenario_listed_here(driver):
    assert subprocess.check_output([driver, "--list"], text=True).split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_plan(driver, scenario):
    p = subprocess.run([driver, scenario], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr


def test_orthographic_variable_is_parsed_whole(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "plugin"), os.path.join(ROOT, "tests", "orthographic_env_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ovrhip_plugin::parse_orthographic(ov" in open(os.path.join(ROOT, "plugin", "device_hip.cpp")).read()
